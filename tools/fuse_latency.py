#!/usr/bin/env python3
"""Per-call latency of the two Fuse loops of LocalMapping::SearchInNeighbors from a C++ caller (tools/native/fuse_latency, built by
__graft_entry__.build()): one 1000-feature key frame into K = 10 / 20 / 60 neighbours, then the neighbours'
points (about 5000 candidates) into that key frame, on the same map restored before every call, alternating in one process so that
drift hits all alike:
  a  ORBmatcher::Fuse called per target as it stands -- the parent's path: the class is unchanged, so this process's library times
     it as the parent commit's does
  b  LocalMapSearch::FuseInTargets / FuseCandidates with points, rows and feature sets resident (the calls also bring the resident
     state up to date with every edit they make)
  c  the same with the feature sets put cold inside the call
  d  the reference's loop restated on the host with the oracle's window search, one core
The program fails unless a, b, c and d return the same counts and leave the same map.  Prints a markdown table: the median over
--runs processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 3
warm-up calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/fuse/first_measurement.md, with the sentence the README row may quote.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("a_orbmatcher", "b_resident", "c_cold_sets", "d_host_loop")


def run_once(prog, n, k, c, reps):
    out = subprocess.run([prog, str(n), str(k), str(c), str(reps)], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("fuse_latency %d %d failed: %s%s" % (n, k, out.stdout, out.stderr))
    r = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0].split("_", 1)[0] in ("targets", "candidates"):
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
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--targets", default="10,20,60")
    ap.add_argument("--candidate-kfs", type=int, default=8)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "fuse_latency")
    lines = ["| pass | targets | points in | fused | a: ORBmatcher us | b: resident us | c: cold sets us | d: host loop us | floor us | b below a by more than the spread |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    faster = []
    for k in [int(x) for x in a.targets.split(",")]:
        runs = [run_once(prog, a.features, k, min(a.candidate_kfs, k), a.reps) for _ in range(a.runs)]
        fl = spread(runs, "floor")
        sh = runs[0]["shape"]
        for form, title, pts, fused in (("targets", "first: into the targets", sh["features"], sh["fused_in_targets"]),
                                        ("candidates", "second: %d key frames' points into one" % sh["candidate_kfs"], sh["candidates"],
                                         sh["fused_candidates"])):
            s = {m: spread(runs, "%s_%s" % (form, m)) for m in MODES}
            ok = s["b_resident"][2] < s["a_orbmatcher"][1]      # the slowest b process under the fastest a process
            faster.append((form, k, ok))
            lines.append("| %s | %d | %d | %d | " % (title, k if form == "targets" else 1, pts, fused) +
                         " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES) + " | %.0f (%.0f-%.0f) | %s |" % (fl + ("yes" if ok else "no",)))
            print(lines[-1], flush=True)
    table = "\n".join(lines)
    slow = ["%s pass at K = %d" % (f, k) for f, k, ok in faster if not ok]
    verdict = ("(b) is below (a) by more than the spread in every row" if not slow else
               "Not faster everywhere: (b) is not below (a) by more than the spread in the " + ", the ".join(slow))
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "fuse"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "fuse", "first_measurement.md"), "w") as f:
            f.write("# Fuse on the resident map, all SearchInNeighbors targets in one call: first measurement\n\n"
                    "`python tools/fuse_latency.py --reps %d --runs %d --write` on one MI355X; median over the processes of the "
                    "per-process medians (smallest - largest of them), microseconds per pass from a C++ caller: the whole first loop of "
                    "SearchInNeighbors over its targets, and the whole second loop.  a - d are described in the tool's header; a is the "
                    "baseline, the path of the parent commit.  Every call of b and c includes the map edits and the updates of the "
                    "resident state that follow them; a and d include the map edits alone.  The floor is `orbhip_debug_roundtrip` mode 1 on "
                    "that box: 4 KB in, an empty kernel, 4 KB out, one synchronisation.  The second pass runs on the map the first pass "
                    "left, with the same candidate key frames in every row.\n\n%s\n\n%s.\n\nNot measured: kernel times (no "
                    "`rocprofv3 --kernel-trace --stats` run), counters, a real sequence.\n" % (a.reps, a.runs, table, verdict))


if __name__ == "__main__":
    main()
