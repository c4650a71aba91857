#!/usr/bin/env python3
"""Per-frame latency of Tracking::UpdateLocalMap + SearchLocalPoints from a C++ caller, host loops against the device path
(tools/native/localcollect_latency, built by __graft_entry__.build()).  Per number of local key frames
(1000-feature rows), alternating in one process so that drift hits all alike:
  a  the host restatement of the reference's two loops on mock objects (the vote of UpdateLocalKeyFrames + its covisibility
     step, UpdateLocalPoints)
  b  a + LocalMapSearch::SearchLocalPoints (orbhip_search_local_points): the baseline, the path the library had before; the
     entry point is unchanged, so this process's library times it as the parent commit's does
  c  orbhip_map_vote + the host graph step + orbhip_track_local_points (LocalMapSearch::UpdateLocalKeyFrames + TrackLocalPoints)
  d  orbhip_map_collect alone
and the cost of keeping the table in step: SetMapPoint of one entry (orbhip_map_kf_set), PutKeyFrame of a 1000-entry row
(orbhip_map_kf_put).  The program fails unless b and c leave the same local map, matches and counts.  Prints a markdown table of
the median over --runs processes of the per-process medians (p10-p90 of the middle process), in microseconds over --reps frames
after 10 warm-up frames; --write puts it into profiles/localmap/collect_first_measurement.md.  Needs the GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("a_host_loops", "b_host_search", "c_device_track", "d_collect", "kf_set_one", "kf_put_1000")
HEAD = ("a: host loops", "b: a + search_local_points", "c: vote + graph + track_local_points", "d: map_collect", "kf_set (1 entry)",
        "kf_put (1000 entries)")


def run_once(prog, kfs, reps):
    out = subprocess.run([prog, str(kfs), str(reps)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("localcollect_latency %d failed: %s%s" % (kfs, out.stdout, out.stderr))
    r = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] in ROWS:
            r[w[0]] = (float(w[2]), float(w[4]), float(w[6]))
        elif w and w[0] == "shape":
            r["shape"] = dict(zip(w[1::2], (int(x) for x in w[2::2])))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", default="20,80,200")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    prog = os.path.join(ROOT, "tools", "native", "localcollect_latency")
    lines = ["| local key frames | local points | in view | " + " | ".join("%s us" % h for h in HEAD) + " | c / b |",
             "|---|---|---|" + "---|" * (len(HEAD) + 1)]
    for kfs in [int(x) for x in a.sizes.split(",")]:
        runs = [run_once(prog, kfs, a.reps) for _ in range(a.runs)]
        cells, med = [], {}
        for k in ROWS:
            by = sorted(runs, key=lambda r: r[k][0])
            mid = by[len(by) // 2][k]
            med[k] = mid[0]
            cells.append("%.0f (%.0f-%.0f)" % mid)
        sh = runs[0]["shape"]
        lines.append("| %d | %d | %d | " % (sh["local_key_frames"], sh["local_points"], sh["in_view"]) + " | ".join(cells) +
                     " | %.2f |" % (med["c_device_track"] / med["b_host_search"]))
        print(lines[-1], flush=True)
    table = "\n".join(lines)
    print(table)
    if a.write:
        verdict = []
        for l in lines[2:]:
            c = [x.strip() for x in l.strip("|").split("|")]
            verdict.append("%s key frames: c is %s x b" % (c[0], c[-1]))
        with open(os.path.join(ROOT, "profiles", "localmap", "collect_first_measurement.md"), "w") as f:
            f.write("# UpdateLocalMap on the device: first measurement\n\n`python tools/localcollect_latency.py --reps %d --runs %d --write` on "
                    "one MI355X; median over the processes of the per-process medians (p10-p90 of the middle process), microseconds "
                    "per frame.  a - d and the two table mutators are described in the tool's header; b is the baseline.  c / b below 1 "
                    "means the device path is faster.\n\n%s\n\n%s.\n\nNot measured: kernel times (no `rocprofv3 --kernel-trace "
                    "--stats` run), counters, a real sequence's map (the synthetic one shares each point among about four key frames).\n"
                    % (a.reps, a.runs, table, "; ".join(verdict)))


if __name__ == "__main__":
    main()
