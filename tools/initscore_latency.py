#!/usr/bin/env python3
"""First measurement of the initialiser's hypothesis scoring -> profiles/initscore/first_measurement.md.

  (a) orbhip_init_score, host form, 200 + 200 hypotheses, N in {300, 1000, 2000} matches: median microseconds per call;
  (b) the same work as the two loops the reference runs, one host thread each (tools/native/initscore_host_loops.c,
      g++ -O3 -march=native -ffp-contract=off, compiled here), timed in the same run; their scores must equal (a)'s bit for bit;
  (c) orbhip_init_score_device, B = 512 problems of N = 1000, everything resident: milliseconds per call from HIP events.
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
NS, NHYP, BATCH, BATCH_N = (300, 1000, 2000), 200, 512, 1000
FLOOR_US = 11.0      # launch + synchronise of an empty call on this machine (profiles/r05/percall_table.md)


def _host_loops():
    src = os.path.join(ROOT, "tools", "native", "initscore_host_loops.c")
    so = os.path.join(tempfile.mkdtemp(prefix="initscore_host_"), "libinitscore_host_loops.so")
    subprocess.check_call(["g++", "-x", "c", "-O3", "-march=native", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.host_score_h.argtypes = [vp, i32, vp, vp, i32, f32, vp, vp, vp]
    L.host_score_f.argtypes = [vp, i32, vp, i32, f32, vp, vp, vp]
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
    import initscore_model as M
    import initscore_scenes as scenes
    from orbhip import initscore
    from orbhip.extractor import ORBextractor
    ex = ORBextractor(500, max_w=320, max_h=240)
    ex._L.orbhip_set_stage_timing(ex.handle, 0)
    HL = _host_loops()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    res = {}
    for N in NS:
        k1, k2, m, Ht = scenes.planar(N, seed=N, extra1=N // 3, extra2=N // 4)
        H21, H12 = scenes.homographies(Ht, NHYP)
        F21 = scenes.fundamentals(scenes.general(50, seed=3)[3], NHYP)
        out = (np.zeros(2 * NHYP, np.float32), np.zeros(2, initscore.BEST_DTYPE), np.zeros(2 * len(k1), np.uint8))
        res["device_us_%d" % N] = _median_us(lambda: initscore.init_score(ex, k1, k2, m, H21, H12, F21, 1.0, out=out), 50, calls)
        idx, u1, v1, u2, v2 = M.pairs(k1, k2, m)
        pr = np.ascontiguousarray(np.stack([u1, v1, u2, v2], 1), np.float32)
        sh, sf = np.zeros(NHYP, np.float32), np.zeros(NHYP, np.float32)
        inl, cur = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        itH, itF = C.c_int(), C.c_int()

        def host_h():
            itH.value = HL.host_score_h(vp(pr), N, vp(H21), vp(H12), NHYP, 1.0, vp(sh), vp(inl), vp(cur))

        def host_f():
            itF.value = HL.host_score_f(vp(pr), N, vp(F21), NHYP, 1.0, vp(sf), vp(inl), vp(cur))
        res["host_h_us_%d" % N] = _median_us(host_h, 5, 40)
        res["host_f_us_%d" % N] = _median_us(host_f, 5, 40)
        assert np.array_equal(np.concatenate([sh, sf]).view(np.uint32), out[0].view(np.uint32)), "host loops and device disagree"
        assert (itH.value, itF.value) == tuple(out[1]["it"])

    # (c) the batched form on resident data
    import hiprt
    rt = hiprt.rt()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    rt.hipEventSynchronize.argtypes = [C.c_void_p]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    k1, k2, m, Ht = scenes.planar(BATCH_N, seed=9, extra1=300, extra2=200)
    H21, H12 = scenes.homographies(Ht, NHYP)
    F21 = scenes.fundamentals(scenes.general(50, seed=3)[3], NHYP)
    n1, n2 = len(k1), len(k2)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (BATCH,) + a.shape))
    bufs = [hiprt.DevBuf.from_numpy(rep(a)) for a in (k1, k2, m, H21, H12, F21)]
    c1, c2 = hiprt.DevBuf.from_numpy(np.full(BATCH, n1, np.int32)), hiprt.DevBuf.from_numpy(np.full(BATCH, n2, np.int32))
    d_s, d_b, d_i = hiprt.DevBuf(BATCH * 2 * NHYP * 4), hiprt.DevBuf(BATCH * 24), hiprt.DevBuf(BATCH * 2 * n1)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0
    stream = ex.stream()
    ms = []
    for i in range(23):
        assert rt.hipEventRecord(e0, stream) == 0
        initscore.init_score_device(ex, bufs[0].ptr, c1.ptr, n1, bufs[1].ptr, c2.ptr, n2, BATCH, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, NHYP,
                                    bufs[5].ptr, NHYP, 1.0, d_s.ptr, d_b.ptr, d_i.ptr)
        assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
        t = C.c_float()
        assert rt.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        if i >= 3:
            ms.append(t.value)
    res["batch_ms"] = statistics.median(ms)
    want = initscore.init_score(ex, k1, k2, m, H21, H12, F21, 1.0)
    got = d_s.to_numpy(np.float32, (BATCH, 2 * NHYP))
    assert np.array_equal(got[BATCH - 1].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[0], got[BATCH // 2])
    for x in bufs + [c1, c2, d_s, d_b, d_i]:
        x.free()
    ex.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initscore", "first_measurement.md"))
    a = ap.parse_args()
    if a.one:
        print("INITSCORE_JSON " + json.dumps(one(a.calls)))
        return
    runs = []
    for _ in range(a.processes):      # a fresh process each: its own context and allocations
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--calls", str(a.calls)], capture_output=True, text=True,
                           timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("INITSCORE_JSON ")]
        if p.returncode != 0 or not line:
            sys.exit("measurement process failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
        runs.append(json.loads(line[0][15:]))
    med = lambda k: statistics.median(r[k] for r in runs)
    spread = lambda k: "%.4g .. %.4g" % (min(r[k] for r in runs), max(r[k] for r in runs))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Initialiser hypothesis scoring: first measurement\n\n`python tools/initscore_latency.py` on one MI355X; %d + %d "
                "hypotheses, planar scenes with a third more frame-1 features than matches.  Medians of %d calls (device) / 40 runs "
                "(host loops) per process; the table gives the median of %d processes and their spread (min .. max).  The host "
                "loops' scores and winners equal the device's bit for bit in every run.  Measured values only.\n\n"
                % (NHYP, NHYP, a.calls, a.processes))
        f.write("| quantity | median of processes | spread |\n|---|---|---|\n")
        for N in NS:
            f.write("| (a) orbhip_init_score, N = %d, us per call | %.4g | %s |\n" % (N, med("device_us_%d" % N), spread("device_us_%d" % N)))
            f.write("| (b) host loop over the %d H hypotheses, one thread, us | %.4g | %s |\n" % (NHYP, med("host_h_us_%d" % N), spread("host_h_us_%d" % N)))
            f.write("| (b) host loop over the %d F hypotheses, one thread, us | %.4g | %s |\n" % (NHYP, med("host_f_us_%d" % N), spread("host_f_us_%d" % N)))
        f.write("| (c) orbhip_init_score_device, B = %d, N = %d, ms per call (HIP events) | %.4g | %s |\n" % (BATCH, BATCH_N, med("batch_ms"), spread("batch_ms")))
        f.write("\n* Launch + synchronise floor of a call on this machine: %.0f us (profiles/r05/percall_table.md); (a) is one upload, three "
                "launches and one synchronisation.\n" % FLOOR_US)
        for N in NS:
            host = max(med("host_h_us_%d" % N), med("host_f_us_%d" % N))
            f.write("* N = %d: the reference runs the two loops on two threads, so its wall time is the longer one, %.0f us; (a) is %.1f us: "
                    "ratio %.1f.\n" % (N, host, med("device_us_%d" % N), host / med("device_us_%d" % N)))
        f.write("* (c) per problem: %.2f us.\n" % (med("batch_ms") * 1e3 / BATCH))
        f.write("* Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run of `tools/initscore_latency.py --one` yet), "
                "counters, other hypothesis counts, and the eight-point solves, which stay on the host and are not part of either side.\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
