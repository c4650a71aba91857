#!/usr/bin/env python3
"""Times the device key-frame database (orbhip/kfdb.py, include/orbhip.h "key-frame database") on ONE MI355X: databases of
1 k / 10 k / 50 k key frames of ~1000 words each over a 10^6-word vocabulary, queries at B = 1 and B = 256.  Prints two
markdown tables (and writes them to --out with the command line and the date):
  1. per database size: the add cost of a key frame without a rebuild, the cost of one rebuild of the inverted file and its
     share per add (delta region of 128), orbhip_kfdb_score (one query: inverted-file walk, counts, scores, reference order
     -- the part the C++ drop-in uses) and orbhip_kfdb_detect (whole reloc / loop queries) as queries per second;
  2. per database size and batch: the device time of each query phase (orbhip_kfdb_phase_times, HIP events) of a reloc call.  Synthetic BowVectors: word ids drawn from a power law, so that some
words are shared by many key frames as in a real vocabulary."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-orb-slam-icra2018_amd"))
import numpy as np  # noqa: E402

from orbhip.extractor import ORBextractor  # noqa: E402
from orbhip.kfdb import KeyFrameDatabase, LOOP, RELOC  # noqa: E402

NWORDS = 1000000


def make_bows(rng, n, words):
    out = []
    for _ in range(n):
        w = np.unique((rng.pareto(0.7, words * 2) * 50).astype(np.int64) % NWORDS)[:words]
        v = rng.random(len(w))
        out.append((w.astype(np.uint32), v / v.sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,50000")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the tables here (markdown)")
    a = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(1)
    ex = ORBextractor(50, 1.2, 1, 20, 7, max_w=128, max_h=128, max_batch=1)
    pool = make_bows(rng, 2000, a.words)
    emit("| key frames | add w/o rebuild (us) | rebuilds | one rebuild (ms) | rebuild per add (us) | score B=1 (q/s) | "
         "reloc B=1 (q/s) | loop B=1 (q/s) | reloc B=256 (q/s) | loop B=256 (q/s) |")
    emit("|---|---|---|---|---|---|---|---|---|---|")
    phases = []
    for N in [int(x) for x in a.sizes.split(",")]:
        db = KeyFrameDatabase(ex, NWORDS, max_kfs=max(N, 1024))
        t_plain = t_fold = 0.0
        n_plain = 0
        for k in range(N):
            r0 = db.info()[3]
            t0 = time.perf_counter()
            db.add(k, pool[k % len(pool)])
            dt = time.perf_counter() - t0
            if db.info()[3] != r0:
                t_fold += dt
            else:
                t_plain += dt
                n_plain += 1
        rebuilds = db.info()[3]
        add_us = t_plain / max(n_plain, 1) * 1e6
        fold_ms = (t_fold / rebuilds * 1e3 - add_us / 1e3) if rebuilds else 0.0   # the add that triggered it, minus an add
        for k in range(0, N, 7):
            db.set_covis(k, [(k + j * 13) % N for j in range(1, 11)])
        qs = [pool[int(i)] for i in rng.integers(0, len(pool), 256)]

        def rate(fn, B, reps):
            fn()                                        # warm-up (allocations)
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            return B * reps / (time.perf_counter() - t)

        r_score = rate(lambda: db.score(RELOC, qs[0]), 1, a.reps)
        r_rel1 = rate(lambda: db.detect(RELOC, qs[:1]), 1, a.reps)
        r_loop1 = rate(lambda: db.detect(LOOP, qs[:1], [[1, 2, 3]], 0.0), 1, a.reps)
        r_rel256 = rate(lambda: db.detect(RELOC, qs), 256, max(1, a.reps // 10))
        r_loop256 = rate(lambda: db.detect(LOOP, qs, [[1, 2, 3]] * 256, 0.0), 256, max(1, a.reps // 10))
        emit("| %d | %.0f | %d | %.2f | %.1f | %.0f | %.0f | %.0f | %.0f | %.0f |" % (
            N, add_us, rebuilds, fold_ms, fold_ms * 1e3 * rebuilds / N, r_score, r_rel1, r_loop1, r_rel256, r_loop256))
        db.set_timing(True)
        for B in (1, 256):
            acc = np.zeros(6)
            for _ in range(5):
                db.detect(RELOC, qs[:B])
                acc += db.phase_times()
            phases.append((N, B, acc / 5))
        db.set_timing(False)
    emit("")
    emit("| key frames | B | walk (ms) | max (ms) | score (ms) | order (ms) | accumulate (ms) | retain + out (ms) |")
    emit("|---|---|---|---|---|---|---|---|")
    for N, B, ms in phases:
        emit("| %d | %d | %s |" % (N, B, " | ".join("%.3f" % x for x in ms)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/kfdb_bench.py\n\n`python3 tools/kfdb_bench.py %s` on %s, %s\n\n" % (
                " ".join(sys.argv[1:]), "one MI355X (gfx950)", time.strftime("%Y-%m-%d")))
            f.write("\n".join(lines) + "\n")
    ex.close()


if __name__ == "__main__":
    main()
