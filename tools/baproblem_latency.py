#!/usr/bin/env python3
"""Per-call latency of the set-up of Optimizer::LocalBundleAdjustment from a C++ caller (tools/native/baproblem_latency, built by
__graft_entry__.build()): a map of 200 key frames of 1000 features, every point seen from about six key
frames of a neighbourhood, the key frame in the middle of the map with its K - 1 nearest key frames as local key frames, K = 10 /
20 / 60, alternating in one process so that drift hits all alike:
  a  the reference's three loops on slamlite.h objects, (pKF, idx) pushed where the reference allocates an edge: the baseline (the
     parent commit has no device path)
  b  LocalMapSearch::BuildLocalBA: one device call, keys and indices turned into pointers, the stamps
  c  orbhip_map_ba_problem alone
The program fails unless the loops and the drop-in give the same five vectors.  Prints a markdown table: the median over --runs
processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 3 warm-up
calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/baproblem/first_measurement.md, with the sentence the README row may quote.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("a_host", "b_dropin", "c_call")


def run_once(prog, k, reps, nkf, nfeat):
    out = subprocess.run([prog, str(k), str(reps), str(nkf), str(nfeat)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("baproblem_latency %d failed: %s%s" % (k, out.stdout, out.stderr))
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
    ap.add_argument("--local", default="10,20,60")
    ap.add_argument("--key-frames", type=int, default=200)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "baproblem_latency")
    lines = ["| K | local points | edges | fixed | a: host loops us | b: BuildLocalBA us | c: orbhip_map_ba_problem us | floor us "
             "| b below a by more than the spread | c below a by more than the spread |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    slow, shape = [], None
    for k in [int(x) for x in a.local.split(",")]:
        runs = [run_once(prog, k, a.reps, a.key_frames, a.features) for _ in range(a.runs)]
        s = {m: spread(runs, m) for m in MODES}
        fl, shape = spread(runs, "floor"), runs[0]["shape"]
        ok_b = s["b_dropin"][2] < s["a_host"][1]               # the slowest b process under the fastest a process
        ok_c = s["c_call"][2] < s["a_host"][1]
        if not ok_b:
            slow.append("(b) at K = %d (a %.0f us, b %.0f us)" % (k, s["a_host"][0], s["b_dropin"][0]))
        if not ok_c:
            slow.append("(c) at K = %d (a %.0f us, c %.0f us)" % (k, s["a_host"][0], s["c_call"][0]))
        lines.append("| %d | %d | %d | %d | " % (k, shape["local_points"], shape["edges"], shape["fixed"]) +
                     " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES) +
                     " | %.0f (%.0f-%.0f) | %s | %s |" % (fl + ("yes" if ok_b else "no", "yes" if ok_c else "no")))
        print(lines[-1], flush=True)
    table = "\n".join(lines)
    verdict = ("(b) and (c) are below (a) by more than the spread in every row" if not slow else
               "**Not faster than the host loops by more than the spread: " + "; ".join(slow) + ".**")
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "baproblem"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "baproblem", "first_measurement.md"), "w") as f:
            f.write("# Local bundle adjustment's problem from the resident key-frame table: first measurement\n\n"
                    "`python tools/baproblem_latency.py --reps %d --runs %d --local %s --write` on one MI355X; median over the processes of "
                    "the per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  The map: %d key "
                    "frames of %d features, %d points, every point seen from the key frames of one neighbourhood; the key frame in the "
                    "middle of the map with its K - 1 nearest key frames are the local key frames.  a - c are described in the tool's "
                    "header; a is the baseline (the reference's three loops on the host objects, pushing (pKF, idx) where the reference "
                    "allocates a g2o edge: the parent commit has no device path).  The floor is `orbhip_debug_roundtrip` mode 1 on that "
                    "box: 4 KB in, an empty kernel, 4 KB out, one synchronisation.\n\n%s\n\n%s.\n\n"
                    "(b) is one `orbhip_map_ba_problem`, or two when the room offered from the last call's sizes was too little, and the "
                    "turning of keys and indices into pointers with the stamps.  Neither side builds a g2o vertex or edge.\n\n"
                    "Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real sequence, maps of other "
                    "sizes, the windowed and the global form.\n"
                    % (a.reps, a.runs, a.local, shape["key_frames"], shape["features"], shape["points"], table, verdict))


if __name__ == "__main__":
    main()
