#!/usr/bin/env python3
"""Per-call latency of ORBmatcher::SearchBySim3 from a C++ caller (tools/native/sim3search_latency, built by
__graft_entry__.build()): the two sides of a loop, two key frames of N = 1000 and of N = 2000 features that see
the same landmarks through a similarity of scale 1.37, about 60 % of the entries of each holding a point, on the same objects,
alternating in one process so that drift hits all alike:
  a  the parent's path: ORBmatcher::SearchBySim3 -- two host projections, two orbhip_window_best_set calls, the agreement on the
     host; the class is unchanged, so this process's library times it as the parent commit's does
  b  LocalMapSearch::SearchBySim3 with points, rows and feature sets resident
  c  orbhip_search_by_sim3 alone, its arguments prepared once
The program fails unless a and b return the same count and leave the same vpMatches12.  Prints a markdown table: the median over
--runs processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 2 warm-up
calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/sim3search/first_measurement.md.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_once(prog, n, reps):
    out = subprocess.run([prog, str(n), str(reps)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("sim3search_latency %d failed: %s%s" % (n, out.stdout, out.stderr))
    r = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0].startswith("sim3_"):
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
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--features", default="1000,2000")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "sim3search_latency")
    lines = ["| features per key frame | points | agreed | a: ORBmatcher us | b: resident us | c: entry point us | floor us | b below a by more than the spread |",
             "|---|---|---|---|---|---|---|---|"]
    slow = []
    for n in [int(x) for x in a.features.split(",")]:
        runs = [run_once(prog, n, a.reps) for _ in range(a.runs)]
        sa, sb, sc, fl = (spread(runs, k) for k in ("sim3_a_orbmatcher", "sim3_b_resident", "sim3_c_entry", "floor"))
        sh = runs[0]["shape"]
        ok = sb[2] < sa[1]                                      # the slowest b process under the fastest a process
        if not ok:
            slow.append("%d features" % n)
        lines.append("| %d | %d | %d | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %s |" %
                     ((n, sh["points"], sh["found"]) + sa + sb + sc + fl + ("yes" if ok else "no",)))
        print(lines[-1], flush=True)
    table = "\n".join(lines)
    verdict = ("(b) is below (a) by more than the spread at both sizes" if not slow else
               "Not faster everywhere: (b) is not below (a) by more than the spread at " + ", ".join(slow))
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "sim3search"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sim3search", "first_measurement.md"), "w") as f:
            f.write("# SearchBySim3 on the resident map: first measurement\n\n"
                    "`python tools/sim3search_latency.py --reps %d --runs %d --write` on one MI355X; median over the processes of the "
                    "per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  Both key frames of a "
                    "pair have the stated number of features; about 60 %% of the entries of each hold a point.  a is the baseline, the "
                    "path of the parent commit (two host projections, two `orbhip_window_best_set` calls, the agreement on the host); "
                    "b is `LocalMapSearch::SearchBySim3` (the taken bytes, one `orbhip_search_by_sim3`, the pointers); c is the entry "
                    "point alone.  The floor is `orbhip_debug_roundtrip` mode 1 on that box: 4 KB in, an empty kernel, 4 KB out, one "
                    "synchronisation.\n\n%s\n\n%s.\n\nNot measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a "
                    "real sequence.\n" % (a.reps, a.runs, table, verdict))


if __name__ == "__main__":
    main()
