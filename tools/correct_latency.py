#!/usr/bin/env python3
"""Per-call latency of CorrectLoop's Sim3 pass and of the global-BA update from a C++ caller (tools/native/correct_latency, built by
__graft_entry__.build()): a map of 200 key frames of 1000 features, K = 10 / 20 / 60 corrected key frames,
alternating in one process so that drift hits all alike:
  loop a  the reference's loop on slamlite.h objects, then LocalMapSearch::Put of the points it moved: the path of the parent commit
          (the class's Put is unchanged, so this process's library times it as the parent commit's does)
  loop b  LocalMapSearch::CorrectLoopPoints: one orbhip_map_correct_sim3 call on the resident store; "entry" is that call alone
  gba a   the reference's global-BA point loop over the whole map, then Put of the points it moved
  gba b   LocalMapSearch::ApplyGlobalBA: one orbhip_map_correct_se3 call; "entry" is that call alone
The program fails unless a and b leave the same positions, normals, distance ranges and poses.  Prints a markdown table: the median
over --runs processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 2
warm-up calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/correct/first_measurement.md.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("loop_a_host_put", "loop_b_correct", "loop_b_entry", "gba_a_host_put", "gba_b_apply", "gba_b_entry")


def run_once(prog, k, reps):
    out = subprocess.run([prog, str(k), str(reps)], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("correct_latency %d failed: %s%s" % (k, out.stdout, out.stderr))
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--corrected", default="10,20,60")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "correct_latency")
    loop = ["| K | points moved | observations | a: host loop + Put us | b: CorrectLoopPoints us | entry point alone us | floor us | b below a by more than the spread |",
            "|---|---|---|---|---|---|---|---|"]
    gba = ["| map points | points moved | a: host loop + Put us | b: ApplyGlobalBA us | entry point alone us | b below a by more than the spread |",
           "|---|---|---|---|---|---|"]
    slow, runs = [], []
    for k in [int(x) for x in a.corrected.split(",")]:
        runs = [run_once(prog, k, a.reps) for _ in range(a.runs)]
        s = {m: spread(runs, m) for m in MODES}
        fl, sh = spread(runs, "floor"), runs[0]["shape"]
        ok = s["loop_b_correct"][2] < s["loop_a_host_put"][1]      # the slowest b process under the fastest a process
        if not ok:
            slow.append("K = %d" % k)
        loop.append("| %d | %d | %d | " % (k, sh["loop_points"], sh["loop_observations"]) +
                    " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES[:3]) + " | %.0f (%.0f-%.0f) | %s |" % (fl + ("yes" if ok else "**not faster**",)))
        print(loop[-1], flush=True)
    s = {m: spread(runs, m) for m in MODES}                         # the map does not depend on K: the last K's processes
    sh = runs[0]["shape"]
    ok = s["gba_b_apply"][2] < s["gba_a_host_put"][1]
    if not ok:
        slow.append("the global-BA update")
    gba.append("| %d | %d | " % (sh["map_points"], sh["gba_points"]) + " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES[3:]) +
               " | %s |" % ("yes" if ok else "**not faster**"))
    table = "\n".join(loop) + "\n\n" + "\n".join(gba)
    verdict = ("(b) is below (a) by more than the spread in every row" if not slow else
               "**Not faster**: (b) is not below (a) by more than the spread at " + ", ".join(slow))
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "correct"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "correct", "first_measurement.md"), "w") as f:
            f.write("# Map points moved on the resident store: first measurement\n\n"
                    "`python tools/correct_latency.py --reps %d --runs %d --corrected %s --write` on one MI355X; median over the processes "
                    "of the per-process medians (smallest - largest of them), microseconds per call from a C++ caller, 200 key frames of "
                    "1000 features.  a and b are described in the tool's header; a is the baseline, the path of the parent commit.  The "
                    "floor is `orbhip_debug_roundtrip` mode 1 on that box: 4 KB in, an empty kernel, 4 KB out, one synchronisation.\n\n%s\n\n%s.\n\n"
                    "(b) contains the host's walk over the key frames' points, the list building (`GetObservations`, the order by `mnId`), "
                    "the entry point, and the assignment of position, normal and range to every object; the entry point alone is the "
                    "packed upload, one launch, one copy back.  What (b) spends outside the entry point is host work on the objects "
                    "(`LocalMapSearch::CorrectTimes()` has the split).\n\n"
                    "Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real sequence.\n"
                    % (a.reps, a.runs, a.corrected, table, verdict))


if __name__ == "__main__":
    main()
