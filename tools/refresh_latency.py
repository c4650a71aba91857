#!/usr/bin/env python3
"""Per-call latency of refreshing one key frame's map points from a C++ caller (tools/native/refresh_latency, built by
__graft_entry__.build()): 1000 points, each seen from about 6 of 20 key frames, all of them recomputed,
alternating in one process so that drift hits all alike:
  a  MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth per point on the host, then LocalMapSearch::Put of all of them:
     the path of the parent commit (the class's Put is unchanged, so this process's library times it as the parent commit's does)
  b  LocalMapSearch::RefreshPoints: one orbhip_map_refresh call on the resident store and feature sets
  c  the host loop alone, without the Put
The program fails unless a and b leave the same descriptors, normals and distance ranges.  Prints a markdown table: the median over
--runs processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 3 warm-up
calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/refresh/first_measurement.md, with the sentence the README row may quote.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("a_host_put", "b_refresh", "c_host_only")


def run_once(prog, n, k, obs, reps):
    out = subprocess.run([prog, str(n), str(k), str(obs), str(reps)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("refresh_latency %d %d %d failed: %s%s" % (n, k, obs, out.stdout, out.stderr))
    r = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in MODES:
            r[w[0]] = float(w[2])
        elif w and w[0] == "floor":
            r["floor"] = float(w[1])
        elif w and w[0] == "shape":
            r["shape"] = dict(zip(w[1::2], (int(x) for x in w[2::2])))
    return r


def spread(runs, k):
    v = sorted(r[k] for r in runs)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--points", default="1000")
    ap.add_argument("--key-frames", type=int, default=20)
    ap.add_argument("--observers", type=int, default=6)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "refresh_latency")
    lines = ["| points | key frames | observations | a: host loop + Put us | b: RefreshPoints us | c: host loop alone us | floor us | b below a by more than the spread |",
             "|---|---|---|---|---|---|---|---|"]
    slow = []
    for n in [int(x) for x in a.points.split(",")]:
        runs = [run_once(prog, n, a.key_frames, a.observers, a.reps) for _ in range(a.runs)]
        s = {m: spread(runs, m) for m in MODES}
        fl, sh = spread(runs, "floor"), runs[0]["shape"]
        ok = s["b_refresh"][2] < s["a_host_put"][1]           # the slowest b process under the fastest a process
        if not ok:
            slow.append("%d points" % n)
        lines.append("| %d | %d | %d | " % (sh["points"], sh["key_frames"], sh["observations"]) +
                     " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES) + " | %.0f (%.0f-%.0f) | %s |" % (fl + ("yes" if ok else "no",)))
        print(lines[-1], flush=True)
    table = "\n".join(lines)
    verdict = ("(b) is below (a) by more than the spread in every row" if not slow else
               "Not faster: (b) is not below (a) by more than the spread at " + ", ".join(slow))
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "refresh"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "refresh", "first_measurement.md"), "w") as f:
            f.write("# Map points refreshed on the resident store: first measurement\n\n"
                    "`python tools/refresh_latency.py --reps %d --runs %d --points %s --write` on one MI355X; median over the processes of "
                    "the per-process medians (smallest - largest of them), microseconds per call from a C++ caller: every point of one key "
                    "frame recomputed -- descriptor, normal, distance range -- and the resident store brought up to date.  a - c are "
                    "described in the tool's header; a is the baseline, the path of the parent commit.  The floor is "
                    "`orbhip_debug_roundtrip` mode 1 on that box: 4 KB in, an empty kernel, 4 KB out, one synchronisation.\n\n%s\n\n%s.\n\n"
                    "Most of (a) is the host loop itself (c): the per-point methods of `slamlite.h` build an N x N matrix and sort every row; the `Put` is the difference between (a) and (c).  (b) contains the host's list building (`GetObservations`, the order by `mnId`, the residency check of the observers' sets), the device call and the assignment of the results.\n\n"
                    "Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real sequence.\n"
                    % (a.reps, a.runs, a.points, table, verdict))


if __name__ == "__main__":
    main()
