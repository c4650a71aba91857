#!/usr/bin/env python3
"""Latency of SearchByBoW against K candidate key frames from a C++ caller (tools/native/bowcand_latency, built by
__graft_entry__.build()): one frame (mode 0, Tracking::Relocalization) or key frame (mode 1,
LoopClosing::ComputeSim3) of 1000 features against K = 1 / 5 / 10 / 20 resident candidates of 1000 features each, 100 vocabulary
nodes (a k = 10 / L = 6 vocabulary at levelsup 4), alternating in one process so that drift hits all alike:
  a  K calls of ORBmatcher::SearchByBoW, in mode 0 each followed by the PnPsolver-constructor loop on the host: the baseline
  b  orbhip_search_by_bow_candidates alone
  c  LocalMapSearch::SearchByBoWCandidates whole
  d  the reference loops on one host core (tests/native_bowcand/ref_bowcand.h)
The program fails unless a, c and d give the same matches.  Prints a markdown table per mode: the median over --runs processes of
the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 3 warm-up calls, and the
floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/bowcand/first_measurement.md.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("a_host", "b_call", "c_dropin", "d_oracle")


def run_once(prog, mode, k, reps, nfeat):
    out = subprocess.run([prog, str(mode), str(k), str(reps), str(nfeat)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("bowcand_latency %d %d failed: %s%s" % (mode, k, out.stdout, out.stderr))
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
    ap.add_argument("--candidates", default="1,5,10,20")
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "bowcand_latency")
    text, slow = [], []
    for mode, what in ((0, "mode 0: SearchByBoW(pKF_k, F) and the PnPsolver arrays (Relocalization)"),
                       (1, "mode 1: SearchByBoW(pCurrentKF, pKF_k) (ComputeSim3)")):
        lines = ["| K | matches | a: K x ORBmatcher::SearchByBoW us | b: orbhip_search_by_bow_candidates us | c: SearchByBoWCandidates us | "
                 "d: reference loops, one core us | floor us | c below a by more than the spreads |", "|---|---|---|---|---|---|---|---|"]
        for k in [int(x) for x in a.candidates.split(",")]:
            runs = [run_once(prog, mode, k, a.reps, a.features) for _ in range(a.runs)]
            s = {m: spread(runs, m) for m in MODES}
            fl, shape = spread(runs, "floor"), runs[0]["shape"]
            ok = s["c_dropin"][2] < s["a_host"][1]            # the slowest c process under the fastest a process
            if not ok:
                slow.append("mode %d, K = %d (a %.0f us, b %.0f us, c %.0f us)" % (mode, k, s["a_host"][0], s["b_call"][0], s["c_dropin"][0]))
            lines.append("| %d | %d | " % (k, shape["matches"]) + " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES) +
                         " | %.0f (%.0f-%.0f) | %s |" % (fl + ("yes" if ok else "**no**",)))
            print(lines[-1], flush=True)
        text.append("## " + what + "\n\n" + "\n".join(lines))
    verdict = ("(c) is below (a) by more than the spreads in every row" if not slow else
               "**Not faster: (c) is not below (a) by more than the spreads at " + "; ".join(slow) + ".**  Of (c), (b) is the device call "
               "with its upload, three kernels and result block; c - b is the drop-in's own work: the check that the store knows every "
               "point of the candidates, the resident-set checks, and the indices turned back into MapPoint*")
    print("\n\n".join(text))
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "bowcand"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "bowcand", "first_measurement.md"), "w") as f:
            f.write("# SearchByBoW against all candidate key frames in one call: first measurement\n\n"
                    "`python tools/bowcand_latency.py --reps %d --runs %d --candidates %s --write` on one MI355X; median over the processes "
                    "of the per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  One frame or key "
                    "frame of %d features against K resident candidates of %d features each, 100 vocabulary nodes; a - d are described in "
                    "the tool's header; a is the baseline, the per-candidate path as it was before this call existed.  The floor is "
                    "`orbhip_debug_roundtrip` mode 1 on that box.\n\n%s\n\n%s.\n\n"
                    "Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real sequence, candidates whose "
                    "sets are not resident yet.\n" % (a.reps, a.runs, a.candidates, a.features, a.features, "\n\n".join(text), verdict))


if __name__ == "__main__":
    main()
