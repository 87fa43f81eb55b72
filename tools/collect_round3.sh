#!/bin/bash
# Round-3 evidence (on the GPU box, from the repo root:  bash tools/collect_round3.sh <commit> ; results land in gpurun_out/r3c/,
# the summaries are then copied into profiles/ by hand):
#   bench.json / bench_{dcunet,convtasnet,demucs}.json   bench lines incl. roofline, cpu_baseline, parity
#   kernel_stats.csv / kernel_stats_serial.csv           rocprofv3 --kernel-trace --stats of the DCCRN bench (overlapped / every kernel alone)
#   kernel_stats_{dcunet,convtasnet,demucs}.csv          the same for the other workloads (overlapped)
#   traffic.json                                         FETCH_SIZE / WRITE_SIZE PMC passes over the real step (tools/traffic_summary.py)
#   mfma_util.json                                       MFMA busy / instruction counters per kernel class (tools/mfma_util_summary.py)
set +e
COMMIT=${1:-unknown}
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$ROOT/gpurun_out/r3c
mkdir -p $OUT
cd $ROOT
timeout 900 python bench.py --full 2>$OUT/bench.err | grep '^{' | tail -1 > $OUT/bench.json
for w in dcunet convtasnet demucs; do
  timeout 600 python bench.py --full --workload $w --steps 20 --warmup 3 2>$OUT/bench_$w.err | grep '^{' | tail -1 > $OUT/bench_$w.json
done
cd /tmp; export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 $ROOT/bench.py --full --steps 30 --warmup 5 --no-cpu-baseline 2>/dev/null | grep '^{' | tail -1 > $OUT/bench_under_rocprof.json
SEHIP_NO_SIDE_STREAM=1 timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_serial -o run -- python3 $ROOT/bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-roofline > /dev/null 2>&1
for w in dcunet convtasnet demucs; do
  timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$w -o run -- python3 $ROOT/bench.py --workload $w --steps 5 --warmup 2 --no-roofline --no-cpu-baseline > /dev/null 2>&1
done
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o run -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > /dev/null 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -o run -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > /dev/null 2>&1
SEHIP_NO_SIDE_STREAM=1 timeout 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS --kernel-trace --output-format csv -d $OUT/pmc_mfmaA -o run -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > /dev/null 2>&1
SEHIP_NO_SIDE_STREAM=1 timeout 600 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --kernel-trace --output-format csv -d $OUT/pmc_mfmaB -o run -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > /dev/null 2>&1
for d in prof prof_serial prof_dcunet prof_convtasnet prof_demucs; do
  f=$(ls $OUT/$d/*/run_kernel_stats.csv $OUT/$d/run_kernel_stats.csv 2>/dev/null | head -1)
  [ -n "$f" ] && cp $f $OUT/kernel_stats${d#prof}.csv
done
t=$(ls $OUT/prof/*/run_kernel_trace.csv $OUT/prof/run_kernel_trace.csv 2>/dev/null | head -1)
cd $ROOT
[ -n "$t" ] && python tools/trace_gaps.py $t > $OUT/gaps.txt 2>&1
python tools/traffic_summary.py $OUT 3 > $OUT/traffic.json 2>$OUT/traffic.err
python tools/mfma_util_summary.py $OUT $COMMIT > $OUT/mfma_util.json 2>$OUT/mfma.err
python - <<PY
import json
p = "$OUT/traffic.json"
try:
    j = json.load(open(p)); j["_whole_step"]["commit"] = "$COMMIT"; json.dump(j, open(p, "w"), indent=1)
except Exception as e:
    print("traffic stamp failed", e)
PY
rm -rf $OUT/prof $OUT/prof_serial $OUT/prof_dcunet $OUT/prof_convtasnet $OUT/prof_demucs $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_mfmaA $OUT/pmc_mfmaB
cut -c1-300 $OUT/bench.json; ls -la $OUT; head -c 1500 $OUT/mfma_util.json
