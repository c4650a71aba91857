#!/usr/bin/env python3
"""Per-call latency of LocalMapping::KeyFrameCulling from a C++ caller (tools/native/cull_latency, built by
__graft_entry__.build()): a map of 200 key frames of 1000 features, every point seen from about six key
frames of a neighbourhood, the K = 20 / 60 key frames in the middle of the map as vpLocalKeyFrames, alternating in one process so
that drift hits all alike:
  a0  the reference loop on slamlite.h objects, 0 culls: the baseline of b (the parent commit has no device path)
  a2  the same with 2 culls: the baseline of c
  b   LocalMapSearch::KeyFrameCulling with 0 culls: one device call
  c   the same with 2 culls: three device calls, two KeyFrameCulled
  d   orbhip_map_cull alone
The program fails unless the loop and the drop-in cull the same key frames.  Prints a markdown table: the median over --runs
processes of the per-process medians, with the smallest and largest of them, in microseconds over --reps calls after 3 warm-up
calls, and the floor of a per-call entry point on that box (orbhip_debug_roundtrip, mode 1).  --write puts it into
profiles/cull/first_measurement.md, with the sentence the README row may quote.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("a0_host", "a2_host", "b_dropin0", "c_dropin2", "d_call")


def run_once(prog, k, reps, nkf, nfeat):
    out = subprocess.run([prog, str(k), str(reps), str(nkf), str(nfeat)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("cull_latency %d failed: %s%s" % (k, out.stdout, out.stderr))
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
    ap.add_argument("--candidates", default="20,60")
    ap.add_argument("--key-frames", type=int, default=200)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "cull_latency")
    lines = ["| K | entries counted | a0: host loop, 0 culls us | a2: host loop, 2 culls us | b: KeyFrameCulling, 0 culls us | c: KeyFrameCulling, 2 culls us "
             "| d: orbhip_map_cull us | floor us | b below a0 by more than the spread | c below a2 by more than the spread |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    slow, shape = [], None
    for k in [int(x) for x in a.candidates.split(",")]:
        runs = [run_once(prog, k, a.reps, a.key_frames, a.features) for _ in range(a.runs)]
        s = {m: spread(runs, m) for m in MODES}
        fl, shape = spread(runs, "floor"), runs[0]["shape"]
        ok_b = s["b_dropin0"][2] < s["a0_host"][1]             # the slowest b process under the fastest a0 process
        ok_c = s["c_dropin2"][2] < s["a2_host"][1]
        if not ok_b:
            slow.append("(b) at K = %d (a0 %.0f us, b %.0f us)" % (k, s["a0_host"][0], s["b_dropin0"][0]))
        if not ok_c:
            slow.append("(c) at K = %d (a2 %.0f us, c %.0f us)" % (k, s["a2_host"][0], s["c_dropin2"][0]))
        lines.append("| %d | %d | " % (k, shape["counted"]) + " | ".join("%.0f (%.0f-%.0f)" % s[m] for m in MODES) +
                     " | %.0f (%.0f-%.0f) | %s | %s |" % (fl + ("yes" if ok_b else "no", "yes" if ok_c else "no")))
        print(lines[-1], flush=True)
    table = "\n".join(lines)
    verdict = ("(b) is below (a0) and (c) below (a2) by more than the spread in every row" if not slow else
               "**Not faster than the host loop by more than the spread: " + "; ".join(slow) + ".**")
    print(table)
    print(verdict)
    if a.write:
        os.makedirs(os.path.join(ROOT, "profiles", "cull"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "cull", "first_measurement.md"), "w") as f:
            f.write("# KeyFrameCulling on the resident key-frame table: first measurement\n\n"
                    "`python tools/cull_latency.py --reps %d --runs %d --candidates %s --write` on one MI355X; median over the processes of "
                    "the per-process medians (smallest - largest of them), microseconds per call from a C++ caller.  The map: %d key "
                    "frames of %d features, %d points with %d observations, every point seen from the key frames of one neighbourhood at "
                    "octaves 0..7, monocular; the K key frames in the middle of the map are vpLocalKeyFrames, two of them redundant.  "
                    "a0 - d are described in the tool's header; a0 and a2 are the baselines (the reference loop on the host objects: the "
                    "parent commit has no device path).  The floor is `orbhip_debug_roundtrip` mode 1 on that box: 4 KB in, an empty "
                    "kernel, 4 KB out, one synchronisation.\n\n%s\n\n%s.\n\n"
                    "(b) is one `orbhip_map_cull` and the check that the store knows every point of the candidates; (c) adds, per cull, "
                    "the caller's `SetBadFlag`, one row erase, one flag upload and one more count of the candidates behind.  The level "
                    "bytes had travelled before the timed calls: in a SLAM run they travel once per key frame.\n\n"
                    "Not measured: kernel times (no `rocprofv3 --kernel-trace --stats` run), counters, a real sequence, maps of other "
                    "sizes, a stereo map, the one-time upload of the level bytes.\n"
                    % (a.reps, a.runs, a.candidates, shape["key_frames"], shape["features"], shape["points"], shape["observations"], table,
                       verdict))


if __name__ == "__main__":
    main()
