#!/bin/bash
# Runs ON THE GPU BOX: everything behind profiles/r04 (one call, one box): the bench line, rocprofv3 kernel stats + HBM counter
# passes of the same command, SQ / GRBM / LDS counter passes, k_fast phase ablation (time, instructions, LDS bank conflicts),
# per-call latencies (Python wrappers incl. the launch + sync floor, and a C++ caller incl. orbhip_frame_build).
# usage: bash tools/r04_profile.sh [tag]          then, in the build container: python tools/update_traffic_meta.py gpurun_out/prof_<tag>
TAG=${1:-r04}
REPO=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$REPO/gpurun_out/prof_$TAG
mkdir -p $OUT
cd $REPO
python bench.py --full > $OUT/bench_stdout.txt 2> $OUT/bench_stderr.txt
tail -1 $OUT/bench_stdout.txt > $OUT/bench.json
bash tools/pmc_gpu.sh util "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU SQ_BUSY_CYCLES" 2>&1 | grep -E "^k_" > $OUT/counters_sq.txt
bash tools/pmc_gpu.sh util2 "GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_SALU SQ_INSTS_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU_MFMA_MOPS_I8 SQ_VALU_MFMA_BUSY_CYCLES" 2>&1 | grep -E "^k_" > $OUT/counters_misc.txt
python3 - "$OUT" <<'PY'
import ast, json, sys
d = sys.argv[1]
def rows(f):
    out = {}
    for l in open(f):
        k, _, v = l.partition(" {")
        out[k.strip()] = ast.literal_eval("{" + v)
    return out
sq, misc = rows(d + "/counters_sq.txt"), rows(d + "/counters_misc.txt")
fast = [k for k in sq if k.startswith("k_fast")][0]
json.dump({"valu_wave_insts_per_launch": int(sq[fast]["SQ_INSTS_VALU"]),
           "grbm_gui_active_per_launch": int(misc[fast]["GRBM_GUI_ACTIVE"]),
           "lds_idx_active_per_launch": int(misc[fast]["SQ_LDS_IDX_ACTIVE"]),
           "lds_bank_conflict_per_launch": int(misc[fast]["SQ_LDS_BANK_CONFLICT"]),
           "valu_source": "profiles/%s/counters_sq.txt (rocprofv3 --pmc SQ_INSTS_VALU ..., own pass)" % d.rsplit("prof_", 1)[-1]},
          open(d + "/fast_valu.json", "w"), indent=1)
PY
bash tools/profile_gpu.sh $TAG > /dev/null 2>&1
python3 - "$OUT" <<'PY'
import json, sys
d = sys.argv[1]
t = json.load(open(d + "/traffic.json"))
if "grbm_gui_active_per_launch" in t and t.get("avg_launch_us"):
    t["clock_ghz"] = round(t["grbm_gui_active_per_launch"] / 8.0 / (t["avg_launch_us"] * 1e-6) / 1e9, 3)
json.dump(t, open(d + "/traffic.json", "w"), indent=1)
PY
bash tools/fast_ablate.sh > $OUT/fast_ablate_time.txt 2>&1
for p in 1 2 3 4 5 8; do
  echo -n "stop<=$p "; ORBHIP_FAST_PHASES=$p bash tools/pmc_gpu.sh ab$p "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT" --steps 2 --warmup 1 --batch 1024 --full --cpu-frames 0 --pipelined 0 --verify 0 --host-batch 0 --configs 0 --content 0 --batch-sweep 0 2>&1 | grep -E "^k_fast"
done > $OUT/fast_ablate_pmc.txt 2>&1
timeout 300 bash tools/pmc_gpu.sh l2 "TCC_HIT_sum TCC_MISS_sum TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum" 2>&1 | grep -E "^k_" > $OUT/counters_l2.txt
python tools/percall_latency.py > $OUT/percall_table.md 2> $OUT/percall_stderr.txt
bash tools/latency_native.sh 3000 > $OUT/latency_native.json 2>&1
bash tools/knn_pmc.sh $TAG > $OUT/knn2_counters.txt 2>&1      # the 4000 x 1M query alone: kernel trace + two counter passes
{ nproc; lscpu | grep 'Model name'; rocm-smi --showclocks 2>/dev/null | head -12; } > $OUT/gpu_box_env.txt 2>&1
cp $OUT/trace/*/*kernel_stats.csv $OUT/kernel_stats.csv 2>/dev/null
find $OUT -name '*.csv' -size +2M -delete
find $OUT -name '*.db' -delete
cat $OUT/bench.json | head -c 1200; echo; cat $OUT/summary.md | head -14
