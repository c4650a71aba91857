#!/usr/bin/env python3
"""First measurement of the PnP / Sim3 hypothesis scoring -> profiles/ransac/first_measurement.md.

  (a) orbhip_pnp_score and orbhip_sim3_score, host forms, N in {100, 500, 2000} correspondences, M = 5 and M = 300 hypotheses:
      median microseconds per call;
  (b) the same work as the loops the reference runs on one host core (tools/native/ransac_host_loops.c, g++ -O3 -march=native
      -ffp-contract=off, compiled here), timed in the same process; their counts and records / winner must equal (a)'s;
  (c) orbhip_pnp_score_device on B = 15 candidates x M = 5 hypotheses at N = 300 -- one round of Tracking::Relocalization --
      everything resident, launch to synchronise, against 15 runs of the host loop.
min_inliers is far above N for Sim3, so that neither side leaves its loop early: both walk all M hypotheses.
Every figure is the median of one process; the table shows three processes and their spread.  `--one` runs one process and prints
its JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vi-orb-slam-icra2018_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
NS, MS, ROUND_B, ROUND_M, ROUND_N = (100, 500, 2000), (5, 300), 15, 5, 300
FLOOR_US = 11.0      # launch + synchronise of an empty call on this machine (profiles/r05/percall_table.md)
i32 = np.int32


def _host_loops():
    src = os.path.join(ROOT, "tools", "native", "ransac_host_loops.c")
    so = os.path.join(tempfile.mkdtemp(prefix="ransac_host_"), "libransac_host_loops.so")
    subprocess.check_call(["g++", "-x", "c", "-O3", "-march=native", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.host_pnp_iterate.argtypes = [vp, i, vp, vp, vp, i, vp, i, i, vp, vp, vp, vp, vp, vp]
    L.host_sim3_iterate.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, i, vp, vp, i, i, vp, vp, vp, vp, vp]
    return L


def _median_us(fn, warm, n):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter_ns()
        fn()
        t.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(t)


def one(calls):
    import ransac_scenes as scenes
    from orbhip import ransac
    from orbhip.extractor import ORBextractor
    ex = ORBextractor(500, max_w=320, max_h=240)
    ex._L.orbhip_set_stage_timing(ex.handle, 0)
    HL = _host_loops()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    res = {}
    for N in NS:
        for Mh in MS:
            host_runs = 200 if Mh == 5 else 20
            # PnP
            s = scenes.pnp(N, Mh, seed=N + Mh)
            X, uv, me, cam, Rt = [np.ascontiguousarray(a) for a in scenes.pnp_args(s)]
            cam = np.asarray(cam, np.float64)
            mi, R = N // 4, min(Mh, 8)
            out = ransac.pnp_score(ex, X, uv, me, cam, Rt, mi, 0, R)
            res["pnp_dev_us_%d_%d" % (N, Mh)] = _median_us(lambda: ransac.pnp_score(ex, X, uv, me, cam, Rt, mi, 0, R, out=out), 50, calls)
            hc, hi, hn = np.zeros(Mh, i32), np.zeros(Mh, i32), np.zeros(Mh, i32)
            cur, bf = np.zeros(max(N, 1), np.uint8), np.zeros(max(N, 1), np.uint8)
            best, nrec = C.c_int(), C.c_int()

            def host_pnp():
                nrec.value = HL.host_pnp_iterate(vp(Rt), Mh, vp(X), vp(uv), vp(me), N, vp(cam), mi, 0, vp(hc), vp(hi), vp(hn), vp(cur), vp(bf),
                                                 C.byref(best))
            res["pnp_host_us_%d_%d" % (N, Mh)] = _median_us(host_pnp, 5, host_runs)
            n = min(nrec.value, R)
            assert np.array_equal(hc, out[0]) and (nrec.value, best.value) == (int(out[1][0]["n_records"]), int(out[1][0]["best_out"]))
            assert np.array_equal(hi[:n], out[2][:n]) and np.array_equal(hn[:n], out[3][:n]), "host loop and device disagree (PnP)"
            # Sim3
            s = scenes.sim3(N, Mh, seed=N + Mh + 1)
            a = [np.ascontiguousarray(v, np.float32) for v in scenes.sim3_args(s)]
            big = 10 ** 6
            out3 = ransac.sim3_score(ex, *a, big, 0)
            res["sim3_dev_us_%d_%d" % (N, Mh)] = _median_us(lambda: ransac.sim3_score(ex, *a, big, 0, out=out3), 50, calls)
            bit = C.c_int()

            def host_sim3():
                nrec.value = HL.host_sim3_iterate(vp(a[8]), Mh, vp(a[0]), vp(a[1]), vp(a[2]), vp(a[3]), vp(a[4]), vp(a[5]), N, vp(a[6]), vp(a[7]),
                                                  big, 0, vp(hc), vp(cur), vp(bf), C.byref(bit), C.byref(best))
            res["sim3_host_us_%d_%d" % (N, Mh)] = _median_us(host_sim3, 5, host_runs)
            r = out3[1][0]
            assert np.array_equal(hc, out3[0]) and (nrec.value, bit.value, best.value) == (int(r["winner"]), int(r["best_it"]), int(r["best_out"])), \
                "host loop and device disagree (Sim3)"

    # (c) one relocalisation round on resident data: B candidates x M hypotheses at N correspondences each
    import hiprt
    B, Mh, N = ROUND_B, ROUND_M, ROUND_N
    ps = [scenes.pnp(N, Mh, seed=900 + b) for b in range(B)]
    cat = lambda k: np.concatenate([np.asarray(s[k], np.float32).reshape(N, -1) for s in ps])
    bufs = [hiprt.DevBuf.from_numpy(cat(k)) for k in ("P3Dw", "P2D", "max_err")] + [hiprt.DevBuf.from_numpy(np.stack([s["Rt"] for s in ps]))]
    off = (np.arange(B + 1) * N).astype(i32)
    mi = np.full(B, N // 4, i32)
    outs = [hiprt.DevBuf(n) for n in (B * Mh * 4, B * 8, B * Mh * 4, B * Mh * 4, Mh * B * N)]

    def round_dev():
        ransac.pnp_score_device(ex, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, off, scenes.CAM, bufs[3].ptr, Mh, mi, None, Mh, *[o.ptr for o in outs])
        ex.sync()
    res["round_dev_us"] = _median_us(round_dev, 50, calls)
    got = outs[0].to_numpy(i32, (B, Mh))
    cam = np.asarray(scenes.CAM, np.float64)
    hc, hi, hn = np.zeros((B, Mh), i32), np.zeros(Mh, i32), np.zeros(Mh, i32)
    cur, bf, best = np.zeros(N, np.uint8), np.zeros(N, np.uint8), C.c_int()
    arrs = [[np.ascontiguousarray(v) for v in scenes.pnp_args(s)] for s in ps]

    def round_host():
        for b, (X, uv, me, _, Rt) in enumerate(arrs):
            HL.host_pnp_iterate(vp(Rt), Mh, vp(X), vp(uv), vp(me), N, vp(cam), int(mi[b]), 0, vp(hc[b]), vp(hi), vp(hn), vp(cur), vp(bf), C.byref(best))
    res["round_host_us"] = _median_us(round_host, 5, 200)
    assert np.array_equal(got, hc), "host loops and device disagree (round)"
    for x in bufs + outs:
        x.free()
    ex.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac", "first_measurement.md"))
    a = ap.parse_args()
    if a.one:
        print("RANSAC_JSON " + json.dumps(one(a.calls)))
        return
    runs = []
    for _ in range(a.processes):      # a fresh process each: its own context and allocations
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--calls", str(a.calls)], capture_output=True, text=True,
                           timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RANSAC_JSON ")]
        if p.returncode != 0 or not line:
            sys.exit("measurement process failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
        runs.append(json.loads(line[0][12:]))
    med = lambda k: statistics.median(r[k] for r in runs)
    spread = lambda k: "%.4g .. %.4g" % (min(r[k] for r in runs), max(r[k] for r in runs))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# PnP / Sim3 hypothesis scoring: first measurement\n\n`python tools/ransac_latency.py` on one MI355X; seeded scenes with 30 %% "
                "outliers, hypotheses from near-perfect to useless.  Medians of %d calls (device) / 200 or 20 runs (host loops, M = 5 / 300) "
                "per process; the table gives the median of %d processes and their spread (min .. max).  The host loops' counts, records "
                "and winners equal the device's in every run.  Sim3 is run with min_inliers above N, so neither side stops early.  "
                "Measured values only.\n\n" % (a.calls, a.processes))
        f.write("| quantity | median of processes | spread |\n|---|---|---|\n")
        for name, key in (("orbhip_pnp_score", "pnp"), ("orbhip_sim3_score", "sim3")):
            for N in NS:
                for Mh in MS:
                    f.write("| (a) %s, N = %d, M = %d, us per call | %.4g | %s |\n" % (name, N, Mh, med("%s_dev_us_%d_%d" % (key, N, Mh)),
                                                                                   spread("%s_dev_us_%d_%d" % (key, N, Mh))))
                    f.write("| (b) host loop, one core, N = %d, M = %d, us | %.4g | %s |\n" % (N, Mh, med("%s_host_us_%d_%d" % (key, N, Mh)),
                                                                                             spread("%s_host_us_%d_%d" % (key, N, Mh))))
        f.write("| (c) orbhip_pnp_score_device, B = %d x M = %d at N = %d, resident, us per call incl. synchronise | %.4g | %s |\n"
                % (ROUND_B, ROUND_M, ROUND_N, med("round_dev_us"), spread("round_dev_us")))
        f.write("| (c) the %d host loops of that round, one core, us | %.4g | %s |\n" % (ROUND_B, med("round_host_us"), spread("round_host_us")))
        f.write("\n* Launch + synchronise floor of a call on this machine: %.0f us (profiles/r05/percall_table.md); (a) is one upload, two "
                "launches and one synchronisation.\n" % FLOOR_US)
        for key in ("pnp", "sim3"):
            for N in NS:
                for Mh in MS:
                    d, h = med("%s_dev_us_%d_%d" % (key, N, Mh)), med("%s_host_us_%d_%d" % (key, N, Mh))
                    f.write("* %s, N = %d, M = %d (M x N = %d): host %.1f us, device %.1f us: host / device = %.2f.\n"
                            % (key, N, Mh, N * Mh, h, d, h / d))
        d, h = med("round_dev_us"), med("round_host_us")
        f.write("* One relocalisation round (B x M x N = %d): host %.1f us, device %.1f us: host / device = %.2f.\n"
                % (ROUND_B * ROUND_M * ROUND_N, h, d, h / d))
        f.write("* Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run of `tools/ransac_latency.py --one` yet), counters, "
                "the EPnP / Horn solves, which stay on the host and are not part of either side, and the device form of Sim3.\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
