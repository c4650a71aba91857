#!/usr/bin/env python3
"""Per-call latency of Tracking::SearchLocalPoints from a C++ caller (tests/native_localmap/test_localmap_dropin in its bench
mode), at the reference's operating point: a 1000-feature 752 x 480 frame and 1000 / 2000 / 4000 / 8000 local points, about half
of them in view.  Per size, alternating in one process so that drift hits all alike:
  host_loop              the isInFrustum loop on one core alone
  per_call_path          that loop + ORBmatcher::SearchByProjection -> orbhip_search_by_projection (what the library did before)
  new_resident_frame     LocalMapSearch::SearchLocalPoints, the frame already a resident set (as after orbhip_set_put_from_frame)
  new_with_frame_upload  the same with the frame's orbhip_set_put inside the call (a frame that was built on the host)
Prints a markdown table (median, 10th and 90th percentile in microseconds over --reps calls after 20 warm-up rounds; --runs
processes per size give the run-to-run spread of the medians), then what LocalMapping pays per touched point (single-point
UpdateFlags / Erase / Put of the class: one upload, one launch, one synchronisation each), then the batched form:
orbhip_search_local_points_device for --batch frames (512) with poses of their own, 2000 local points each, against one store --
milliseconds per call and frames/s over --batch-reps calls after 5 warm-up calls, each call timed to its orbhip_sync.
Needs the GPU."""
import ctypes as C
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("vi-orb-slam-icra2018_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", default="1000,2000,4000,8000")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--batch-reps", type=int, default=30)
    a = ap.parse_args()
    import orb_oracle_py as oracle
    import localmap_scenes as scenes
    from localmap_scenes import write_scene
    oracle.build()
    prog = os.path.join(ROOT, "tests", "native_localmap", "test_localmap_dropin")
    rows = ("host_loop", "per_call_path", "new_resident_frame", "new_with_frame_upload")
    print("| local points | in view | " + " | ".join("%s median (p10-p90) us" % r for r in rows) + " | medians of the runs, per_call / new_resident |")
    print("|---|---|" + "---|" * (len(rows) + 1))
    single = ("update_flags_one", "erase_one", "put_one")
    store_rows = []
    for nq in [int(x) for x in a.sizes.split(",")]:
        sc = scenes.make(oracle, "752x480", npoints=nq)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "scene.bin")
            write_scene(path, sc, 1.0, np.zeros(nq, np.uint8), sc["occupied"])
            runs = []
            for _ in range(a.runs):
                out = subprocess.run([prog, path, "bench", str(a.reps)], capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    sys.exit("bench run failed: " + out.stdout + out.stderr)
                r = {}
                for line in out.stdout.splitlines():
                    w = line.split()
                    if w[0] in rows or w[0] in single:
                        r[w[0]] = (float(w[2]), float(w[4]), float(w[6]))
                    elif w[0] == "n_to_match":
                        r["ntm"] = int(w[1])
                    elif w[0] == "put_all":
                        r["put_all"] = float(w[3])
                runs.append(r)
        mid = runs[len(runs) // 2]
        spread = "%s / %s" % ("-".join("%.0f" % x for x in sorted(r["per_call_path"][0] for r in runs)),
                              "-".join("%.0f" % x for x in sorted(r["new_resident_frame"][0] for r in runs)))
        print("| %d | %d | " % (nq, mid["ntm"]) + " | ".join("%.0f (%.0f-%.0f)" % mid[k] for k in rows) + " | " + spread + " |", flush=True)
        store_rows.append("| %d | " % nq + " | ".join("%.0f (%.0f-%.0f)" % mid[k] for k in single) + " | %.0f |" % mid["put_all"])
    print()
    print("| points in the store | UpdateFlags(one point) us | Erase(one point) us | Put(one point) us | Put(all points, one call) us |")
    print("|---|---|---|---|---|")
    print("\n".join(store_rows), flush=True)
    if a.batch > 0:
        batched(oracle, scenes, a.batch, a.batch_reps)


def batched(oracle, scenes, B, reps, nq=2000):
    """orbhip_search_local_points_device: B copies of the scene's frame, each with a pose of its own, one store."""
    import time
    from orbhip import capi, localmap
    from orbhip.capi import check
    from orbhip.extractor import ORBextractor
    sc = scenes.make(oracle, "752x480", npoints=nq)
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    L, h = ex._L, ex.handle
    rt = C.CDLL("libamdhip64.so.7")       # (already in the process: liborbhip.so links it)
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    rt.hipFree.argtypes = [C.c_void_p]
    bufs = []

    def dev(arr=None, nbytes=0):
        p = C.c_void_p()
        n = arr.nbytes if arr is not None else nbytes
        assert rt.hipMalloc(C.byref(p), max(n, 16)) == 0 and rt.hipMemset(p, 0, max(n, 16)) == 0
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            assert rt.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        bufs.append(p)
        return p

    lm = localmap.LocalMap(ex, nq)
    lm.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
    rng = np.random.default_rng(1)
    n = len(sc["kps"])
    cap = n
    cams = np.zeros(B, localmap.CAMERA_DTYPE)
    cam = sc["cam"]
    for b in range(B):
        R, t, Ow = scenes.pose(rng)
        cams[b] = localmap.camera(R, t, Ow, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"], cam["scale_factors"],
                                  cam["log_scale_factor"], cam["viewing_cos_limit"], 1.0)[0]
    slots = np.tile(lm.slots(sc["keys"]), (B, 1))
    d_kps, d_desc = dev(np.tile(sc["kps"], (B, 1))), dev(np.tile(sc["desc"], (B, 1, 1)))
    d_cnt, d_occ = dev(np.full(B, n, np.int32)), dev(np.tile(sc["occupied"], (B, 1)))
    d_off, d_idx = dev(nbytes=B * (64 * 48 + 1) * 4), dev(nbytes=B * cap * 4)
    d_cam, d_slots, d_skip, d_nq = dev(lm.prepare(cams)), dev(slots), dev(np.zeros((B, nq), np.uint8)), dev(np.full(B, nq, np.int32))
    d_pts, d_ntm, d_m, d_nm = dev(nbytes=B * nq * 24), dev(nbytes=B * 4), dev(nbytes=B * cap * 4), dev(nbytes=B * 4)
    gp = sc["gp"]
    check(L.orbhip_grid_build_device(h, d_kps, d_cnt, cap, B, gp[0], gp[1], gp[2], gp[3], d_off, d_idx), h, "grid")
    ex.sync()
    ms = []
    for it in range(reps + 5):
        t0 = time.perf_counter()
        check(L.orbhip_search_local_points_device(h, d_kps, d_desc, d_cnt, cap, B, None, d_occ, gp[0], gp[1], gp[2], gp[3], d_off, d_idx,
                                                  d_cam, d_slots, d_skip, d_nq, nq, 0.8, d_pts, d_ntm, d_m, d_nm), h, "search")
        ex.sync()
        if it >= 5:
            ms.append((time.perf_counter() - t0) * 1e3)
    ntm = np.zeros(B, np.int32)
    nm = np.zeros(B, np.int32)
    assert rt.hipMemcpy(ntm.ctypes.data, d_ntm, ntm.nbytes, 2) == 0 and rt.hipMemcpy(nm.ctypes.data, d_nm, nm.nbytes, 2) == 0
    ms.sort()
    med = ms[len(ms) // 2]
    print()
    print("| batched form | frames | local points per frame | in view (mean) | matches (mean) | ms per call median (p10-p90) | frames/s | us per frame |")
    print("|---|---|---|---|---|---|---|---|")
    print("| orbhip_search_local_points_device | %d | %d | %.0f | %.0f | %.2f (%.2f-%.2f) | %.0f | %.1f |" %
          (B, nq, ntm.mean(), nm.mean(), med, ms[len(ms) // 10], ms[len(ms) * 9 // 10], B / med * 1e3, med * 1e3 / B), flush=True)
    ex.close()
    for p in bufs:
        rt.hipFree(p)


if __name__ == "__main__":
    main()
