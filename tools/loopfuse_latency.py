#!/usr/bin/env python3
"""Per-call latency of LoopClosing's two projection searches from a C++ caller (tools/native/loopfuse_latency, built by
__graft_entry__.build()): SearchAndFuse of about 4000 loop points (the union of 8 key frames of 1000
features) into K = 10 / 20 / 60 corrected key frames, and SearchLoopPoints of the same list into one key frame, on the same map
restored before every call, alternating in one process so that drift hits both alike:
  a  the parent's path: ORBmatcher::Fuse(pKF, Scw, ...) per key frame with the Replace loop, respectively the union on the host
     and ORBmatcher::SearchByProjection(pKF, Scw, ...) -- the class is unchanged, so this process's library times it as the parent
     commit's does
  b  LocalMapSearch::SearchAndFuse / SearchLoopPoints with points, rows and feature sets resident (SearchAndFuse also brings the
     resident state up to date with every edit it makes)
The program fails unless a and b leave the same map and the same matches.  Prints a markdown table: the median over --runs
processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 2 warm-up
calls, the phase clock of b's SearchAndFuse (preparation / device call / second searches / apply / resident state, per call), and
the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/loopfuse/first_measurement.md.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ("prepare", "device", "research", "apply", "resident")


def run_once(prog, n, k, l, reps):
    out = subprocess.run([prog, str(n), str(k), str(l), str(reps)], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("loopfuse_latency %d %d failed: %s%s" % (n, k, out.stdout, out.stderr))
    r = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0].split("_", 1)[0] in ("looppoints", "fuse"):
            r[w[0]] = float(w[2])
        elif w and w[0] == "phase":
            r["phase_" + w[1]] = float(w[2])
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
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--targets", default="10,20,60")
    ap.add_argument("--loop-kfs", type=int, default=8)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "loopfuse_latency")
    lines = ["| call | key frames | loop points | a: ORBmatcher us | b: resident us | floor us | b below a by more than the spread |", "|---|---|---|---|---|---|---|"]
    phases = ["| K | " + " | ".join(PHASES) + " |", "|---|" + "---|" * len(PHASES)]
    verdicts = []
    for k in [int(x) for x in a.targets.split(",")]:
        runs = [run_once(prog, a.features, k, a.loop_kfs, a.reps) for _ in range(a.runs)]
        fl = spread(runs, "floor")
        sh = runs[0]["shape"]
        for form, title, kfs in (("fuse", "SearchAndFuse", k), ("looppoints", "SearchLoopPoints", 1)):
            if form == "looppoints" and verdicts and any(v[0] == form for v in verdicts):
                continue                                        # the same call in every row: reported once
            sa, sb = spread(runs, form + "_a_orbmatcher"), spread(runs, form + "_b_resident")
            ok = sb[2] < sa[1]                                  # the slowest b process under the fastest a process
            verdicts.append((form, k, ok))
            lines.append("| %s | %d | %d | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %s |" %
                         ((title, kfs, sh["loop_points"]) + sa + sb + fl + ("yes" if ok else "no",)))
            print(lines[-1], flush=True)
        phases.append("| %d | " % k + " | ".join("%.0f" % spread(runs, "phase_" + p)[0] for p in PHASES) + " |")
    table, ptable = "\n".join(lines), "\n".join(phases)
    slow = ["%s at %d key frames" % (f, k) for f, k, ok in verdicts if not ok]
    verdict = ("(b) is below (a) by more than the spread in every row" if not slow else
               "Not faster everywhere: (b) is not below (a) by more than the spread for " + ", ".join(slow))
    print(table)
    print(ptable)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "loopfuse"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "loopfuse", "first_measurement.md"), "w") as f:
            f.write("# LoopClosing's projection searches on the resident map: first measurement\n\n"
                    "`python tools/loopfuse_latency.py --reps %d --runs %d --write` on one MI355X; median over the processes of the "
                    "per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  a is the baseline, the "
                    "path of the parent commit; b includes the map edits and the updates of the resident state that follow them, a the map "
                    "edits alone.  The floor is `orbhip_debug_roundtrip` mode 1 on that box: 4 KB in, an empty kernel, 4 KB out, one "
                    "synchronisation.\n\n%s\n\nWhere b's SearchAndFuse spends its time (microseconds per call, median over the processes): "
                    "preparation, the device call, the second searches of changed survivors, the apply and Replace loops, the resident "
                    "state.\n\n%s\n\n%s.\n\nNot measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real "
                    "sequence.\n" % (a.reps, a.runs, table, ptable, verdict))


if __name__ == "__main__":
    main()
