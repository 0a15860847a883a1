#!/bin/bash
# Round artefacts in one box session: PMC traffic table -> bench (--full) -> rocprof kernel stats / pass breakdowns -> serving.
# Usage: tools/run_final.sh OUT_DIR
OUT=${1:?usage: tools/run_final.sh OUT_DIR}
cd $GRAFT_REPO_ROOT
bash tools/pmc_traffic.sh > gpurun_out/pmc_traffic.log 2>&1 || { tail -20 gpurun_out/pmc_traffic.log; exit 1; }
tail -3 gpurun_out/pmc_traffic.log
cp gpurun_out/r02_traffic.json profiles/r02_traffic.json
bash tools/final_profiles.sh $OUT/final > $OUT/final_profiles.log 2>&1 || { tail -20 $OUT/final_profiles.log; exit 2; }
cut -c1-300 $OUT/final/bench.json
LCM_BENCH_ONE_DEVICE=1 timeout -k 10 300 python bench.py --gpus 2 --steps 10 --full --no-cpu-baseline --no-extra > $OUT/final/bench_2ranks_one_device.json 2> $OUT/final/bench_2ranks.err; cut -c1-300 $OUT/final/bench_2ranks_one_device.json
timeout -k 10 300 python bench.py --model sdxl --no-cpu-baseline --no-extra --no-roofline --steps 3 --warmup 1 > $OUT/final/bench_sdxl.json 2>/dev/null; cut -c1-200 $OUT/final/bench_sdxl.json
timeout -k 10 300 python bench.py --size 768 --lcm-steps 8 --batch 8 --no-cpu-baseline --no-extra --no-roofline --steps 3 --warmup 1 > $OUT/final/bench_768.json 2>/dev/null; cut -c1-200 $OUT/final/bench_768.json
timeout -k 10 400 python tools/worker_latency.py > $OUT/final/worker_latency.txt 2>&1; grep -E "callers|png level|sampler only" $OUT/final/worker_latency.txt
