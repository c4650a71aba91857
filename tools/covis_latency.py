#!/usr/bin/env python3
"""Per-call latency of updating the covisibility graph from a C++ caller (tools/native/covis_latency, built by
__graft_entry__.build()): a map of 200 key frames of 1000 features, every point seen from about six key
frames of a neighbourhood, K = 1 / 10 / 20 / 60 key frames in the middle of the map updated back to back, alternating in one
process so that drift hits all alike:
  a  sequential KeyFrame::UpdateConnections of slamlite.h on the host objects: the baseline
  b  orbhip_map_covis alone: counts, weights and orders, nothing applied
  c  LocalMapSearch::UpdateConnections whole: the call, then AddConnection, the lists and the parent on the caller's objects
The graph is emptied before every timed call, so a and c do the same per-neighbour AddConnection / UpdateBestCovisibles work; the
program fails unless a and c leave the same graph.  Prints a markdown table: the median over --runs processes of the per-process
medians, with the smallest and largest of them, in microseconds over --reps calls after 3 warm-up calls, and the floor of a
per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into profiles/covis/first_measurement.md, with
the sentence the README row may quote.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("a_host", "b_call", "c_dropin")


def run_once(prog, k, reps, nkf, nfeat):
    out = subprocess.run([prog, str(k), str(reps), str(nkf), str(nfeat)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("covis_latency %d failed: %s%s" % (k, out.stdout, out.stderr))
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
    ap.add_argument("--queries", default="1,10,20,60")
    ap.add_argument("--key-frames", type=int, default=200)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "covis_latency")
    lines = ["| K | links of the K | a: host UpdateConnections us | b: orbhip_map_covis us | c: LocalMapSearch::UpdateConnections us | c - b us | floor us | c below a by more than the spread |",
             "|---|---|---|---|---|---|---|---|"]
    slow, shape = [], None
    for k in [int(x) for x in a.queries.split(",")]:
        runs = [run_once(prog, k, a.reps, a.key_frames, a.features) for _ in range(a.runs)]
        s = {m: spread(runs, m) for m in MODES}
        fl, shape = spread(runs, "floor"), runs[0]["shape"]
        ok = s["c_dropin"][2] < s["a_host"][1]                # the slowest c process under the fastest a process
        if not ok:
            slow.append("K = %d (a %.0f us, b %.0f us, c %.0f us)" % (k, s["a_host"][0], s["b_call"][0], s["c_dropin"][0]))
        lines.append("| %d | %d | " % (k, shape["links"]) + " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES) +
                     " | %.0f | %.0f (%.0f-%.0f) | %s |" % ((s["c_dropin"][0] - s["b_call"][0],) + fl + ("yes" if ok else "no",)))
        print(lines[-1], flush=True)
    table = "\n".join(lines)
    verdict = ("(c) is below (a) by more than the spread in every row" if not slow else
               "**Not faster: (c) is not below (a) by more than the spread at " + "; ".join(slow) + ".**  Of (c), (b) is the device "
               "call with its upload, sweeps, result block and the host's ordering; c - b is the drop-in's own work: the check that the "
               "store knows every point of the key frames, and the AddConnection / UpdateBestCovisibles calls on the neighbours, which "
               "(a) pays as well")
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "covis"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "covis", "first_measurement.md"), "w") as f:
            f.write("# The covisibility graph from the resident key-frame table: first measurement\n\n"
                    "`python tools/covis_latency.py --reps %d --runs %d --queries %s --write` on one MI355X; median over the processes of "
                    "the per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  The map: %d key "
                    "frames of %d features, %d points with %d observations, every point seen from the key frames of one neighbourhood; "
                    "the K key frames in the middle of the map are updated back to back, from an empty graph.  a - c are described in the "
                    "tool's header; a is the baseline.  The floor is `orbhip_debug_roundtrip` mode 1 on that box: 4 KB in, an empty "
                    "kernel, 4 KB out, one synchronisation.\n\n%s\n\n%s.\n\n"
                    "The per-neighbour `UpdateBestCovisibles` sorts stay on the host in both paths.  (a) walks a copy of every point's "
                    "observation map; its cost grows with K.  (b) sweeps the whole table once per 32 queries whatever K is.\n\n"
                    "Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real sequence, maps of other "
                    "sizes, a graph that is already built (where most `AddConnection` calls return at once).\n"
                    % (a.reps, a.runs, a.queries, shape["key_frames"], shape["features"], shape["points"], shape["observations"], table,
                       verdict))


if __name__ == "__main__":
    main()
