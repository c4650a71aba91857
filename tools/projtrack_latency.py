#!/usr/bin/env python3
"""Per-call latency of Tracking's two other projection searches from a C++ caller (tools/native/projtrack_latency, built by
__graft_entry__.build()), at N source points against an N-feature 752 x 480 frame, for
SearchByProjection(CurrentFrame, LastFrame, ...) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, ...), alternating in one
process so that drift hits all alike:
  a  ORBmatcher's method as it stands -- the parent's path: the class is unchanged, so this process's library times it as the
     parent commit's does
  b  LocalMapSearch::SearchLastFrame / SearchKeyFramePoints with frames, points and row resident
  c  the same with the frames' sets put cold inside the call
  d  the restated host loop with the oracle's window search, one core
The program fails unless a, b, c and d leave the same matches and counts.  Prints a markdown table: the median over --runs
processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 10 warm-up
calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/projtrack/first_measurement.md, with the sentence the README row may quote.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("last_a_orbmatcher", "last_b_resident", "last_c_cold_sets", "last_d_host_loop",
        "kf_a_orbmatcher", "kf_b_resident", "kf_c_cold_sets", "kf_d_host_loop")


def run_once(prog, n, reps):
    out = subprocess.run([prog, str(n), str(reps)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("projtrack_latency %d failed: %s%s" % (n, out.stdout, out.stderr))
    r = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in ROWS:
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="1000,2000")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "projtrack_latency")
    lines = ["| search | N | matches | a: ORBmatcher us | b: resident us | c: cold sets us | d: host loop us | floor us | b below a by more than the spread |",
             "|---|---|---|---|---|---|---|---|---|"]
    faster = []
    for n in [int(x) for x in a.sizes.split(",")]:
        runs = [run_once(prog, n, a.reps) for _ in range(a.runs)]
        fl = spread(runs, "floor")
        for form, title in (("last", "last frame"), ("kf", "key frame")):
            s = {k: spread(runs, "%s_%s" % (form, k)) for k in ("a_orbmatcher", "b_resident", "c_cold_sets", "d_host_loop")}
            ok = s["b_resident"][2] < s["a_orbmatcher"][1]      # the slowest b process under the fastest a process
            faster.append(ok)
            lines.append("| %s | %d | %d | " % (title, n, runs[0]["shape"]["%s_matches" % form]) +
                         " | ".join("%.0f (%.0f-%.0f)" % s[k] for k in ("a_orbmatcher", "b_resident", "c_cold_sets", "d_host_loop")) +
                         " | %.0f (%.0f-%.0f) | %s |" % (fl + ("yes" if ok else "no",)))
            print(lines[-1], flush=True)
    table = "\n".join(lines)
    verdict = ("(b) is below (a) by more than the spread at every size, for both searches" if all(faster) else
               "Not faster: (b) is not below (a) by more than the spread at every size")
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "projtrack"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "projtrack", "first_measurement.md"), "w") as f:
            f.write("# Last-frame and key-frame projection searches on the resident map: first measurement\n\n"
                    "`python tools/projtrack_latency.py --reps %d --runs %d --write` on one MI355X; median over the processes of the "
                    "per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  a - d are described in "
                    "the tool's header; a is the baseline, the path of the parent commit.  The floor is `orbhip_debug_roundtrip` mode 1 "
                    "on that box: 4 KB in, an empty kernel, 4 KB out, one synchronisation.\n\n%s\n\n%s.\n\nNot measured: kernel times (no "
                    "`rocprofv3 --kernel-trace --stats` run), counters, a real sequence.\n" % (a.reps, a.runs, table, verdict))


if __name__ == "__main__":
    main()
