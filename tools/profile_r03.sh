#!/bin/bash
# Round-3 profiling recipe, run ON THE GPU BOX (via gpurun).  Usage: tools/profile_r03.sh <tag>
#  1. kernel trace + stats of the default bench (per-kernel average durations)
#  2. separate PMC passes FETCH_SIZE / WRITE_SIZE (TCC slots cannot hold both) on a decode-only run
#     and on a GRM-only run (cfg4 shape, 2 launches of 62500 SNPs), for HBM traffic per launch
#  3. one SQ pass on the GRM-only run: MFMA busy per SIMD and the loaded clock
# Every step has its own time limit and the chain stops at the first failure.
set -e
TAG=${1:-r03}
OUT=gpurun_out/prof_$TAG
mkdir -p $OUT
export TMPDIR=/tmp
DEC="--full --steps 1 --warmup 1 --skip-cpu --skip-grm --grm5 off --e2e off --beta off --file off"
GRM="--full --n-iid 16384 --n-sid 16384 --steps 1 --warmup 0 --skip-cpu --grm-sid 125000 --grm-f64 off --grm5 off --e2e off --beta off --file off"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- python3 bench.py --full --skip-cpu > $OUT/bench_under_rocprof.json 2> $OUT/trace.log
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 120 rocprofv3 --pmc $C --kernel-trace -d $OUT/dec_$C -o run --output-format csv -- python3 bench.py $DEC > $OUT/dec_$C.log 2>&1
  timeout -s KILL 120 rocprofv3 --pmc $C --kernel-trace -d $OUT/grm_$C -o run --output-format csv -- python3 bench.py $GRM > $OUT/grm_$C.log 2>&1
done
timeout -s KILL 120 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE --kernel-trace -d $OUT/grm_SQ -o run --output-format csv -- python3 bench.py $GRM > $OUT/grm_SQ.log 2>&1
python3 tools/traffic_summary.py $OUT $OUT/traffic.json 500000,2048 50000,62500 > $OUT/traffic.log 2>&1 || true
python3 tools/pmc_summary.py $OUT/grm_SQ --match k_syrk > $OUT/pmc_sq_grm.json 2>&1 || true
echo profile-done
