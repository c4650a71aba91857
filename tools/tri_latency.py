#!/usr/bin/env python3
"""First measurement of SearchForTriangulation on resident sets -> profiles/triangulation/first_measurement.md.

tools/native/tri_latency (a C++ caller of the C ABI) matches one key frame of 1000 features against K = 10 and K = 20 neighbours of
1000 features, in one process on the same inputs, after comparing the results of all four for equality:
  (a) K orbhip_search_for_triangulation calls -- the upload-per-call path, the baseline;
  (b) one orbhip_search_for_triangulation_sets call with the K + 1 sets resident;
  (c) the same with the sets put cold (drop, K + 1 orbhip_set_put, the call);
  (d) the oracle's loop on one host core, K times.
Every figure is the median of one process; the table shows the median of several processes and their spread.
`--one` runs one process and prints its JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "native", "tri_latency")
ORACLE = os.path.join(ROOT, "oracle", "liborb_oracle.so")
FLOOR_US = 11.0      # launch + synchronise of an empty call on this machine (profiles/r05/percall_table.md)
ROWS = (("single_us", "(a) K orbhip_search_for_triangulation calls"), ("batched_us", "(b) one orbhip_search_for_triangulation_sets call, sets resident"),
        ("cold_us", "(c) the same, sets put cold (drop + K + 1 orbhip_set_put + the call)"), ("oracle_us", "(d) the oracle, one host core, K calls"))


def one(calls):
    for p in (TOOL, ORACLE):
        if not os.path.exists(p):
            sys.exit("%s is not built (run __graft_entry__.build())" % p)
    p = subprocess.run([TOOL, ORACLE, str(calls)], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("TRI_JSON ")]
    if p.returncode != 0 or not line:
        sys.exit("tri_latency failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
    return json.loads(line[0][9:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulation", "first_measurement.md"))
    a = ap.parse_args()
    if a.one:
        print("TRI_JSON " + json.dumps(one(a.calls)))
        return
    runs = [one(a.calls) for _ in range(a.processes)]      # a fresh process each: its own context and allocations
    med = lambda K, k: statistics.median(r[K][k] for r in runs)
    lo = lambda K, k: min(r[K][k] for r in runs)
    hi = lambda K, k: max(r[K][k] for r in runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# SearchForTriangulation on resident sets: first measurement\n\n`python tools/tri_latency.py` on one MI355X: one key frame "
                "of 1000 features against K neighbours of 1000 features (synthetic views of one set of features, ~100 shared vocabulary "
                "nodes, ~60 %% stereo features, 30 %% of the features skipped), from a C++ caller.  The four rows of a K are timed in the same "
                "process on the same inputs, and their match rows are compared for equality before anything is timed.  Medians of %d calls "
                "((a), (b)) / %d runs ((c), (d)) per process; the table gives the median of %d processes and their spread (min .. max).  "
                "Measured values only.\n\n" % (a.calls, max(10, a.calls // 10), a.processes))
        f.write("| K | quantity | median of processes, us | spread, us |\n|---|---|---|---|\n")
        for K in ("K10", "K20"):
            for key, name in ROWS:
                f.write("| %s | %s | %.4g | %.4g .. %.4g |\n" % (K[1:], name, med(K, key), lo(K, key), hi(K, key)))
        f.write("\n")
        for K in ("K10", "K20"):
            f.write("* K = %s: %d matches over the neighbours.  " % (K[1:], runs[0][K]["matches"]))
            gap = lo(K, "single_us") - hi(K, "batched_us")
            if gap > 0:
                f.write("(b) is below (a) in every process: the slowest (b), %.4g us, is %.4g us under the fastest (a), %.4g us; medians "
                        "(a) / (b) = %.2f.\n" % (hi(K, "batched_us"), gap, lo(K, "single_us"), med(K, "single_us") / med(K, "batched_us")))
            else:
                f.write("(b) is NOT below (a) by more than the run-to-run spread: (a) %.4g .. %.4g us, (b) %.4g .. %.4g us.  No gain is "
                        "claimed.\n" % (lo(K, "single_us"), hi(K, "single_us"), lo(K, "batched_us"), hi(K, "batched_us")))
        f.write("* Launch + synchronise floor of a call on this machine: %.0f us (profiles/r05/percall_table.md); (a) pays it K times, (b) "
                "once.\n" % FLOOR_US)
        f.write("* Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run of `tools/native/tri_latency` yet), counters, the "
                "drop-in class's host work (set identity checks, flags), and the triangulation that follows, which stays on the host.\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
