#!/bin/bash
# Regenerates the round's judged artefacts in ONE box session: bench JSON (--full), then the plain bench command under
# rocprofv3 --kernel-trace --stats for batch 1 and batch 8 (tuning plans cached so all three runs use the same plans).
# Usage: tools/final_profiles.sh OUT_DIR
set -o pipefail
OUT=${1:?usage: tools/final_profiles.sh OUT_DIR}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export LCM_TUNE_CACHE=/tmp/tc.json
mkdir -p $OUT
timeout -k 10 700 python3 bench.py --full > $OUT/bench.json 2> $OUT/bench.err || exit 1
echo "bench done" && cat $OUT/bench.json | cut -c1-400
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/b1 -- python3 bench.py --no-cpu-baseline --no-extra --no-roofline > $OUT/b1_bench.json 2> $OUT/b1.err || exit 2
echo "b1 prof done"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/b8 -- python3 bench.py --batch 8 --no-cpu-baseline --no-extra --no-roofline > $OUT/b8_bench.json 2> $OUT/b8.err || exit 3
echo "b8 prof done"
for t in b1 b8; do
  f=$(find $OUT/$t -name "*kernel_stats.csv" | head -1)
  cp "$f" $OUT/${t}_kernel_stats.csv
  python tools/pass_breakdown.py $OUT/$t 60 > $OUT/${t}_pass_breakdown.txt
  python tools/pass_sequence.py $OUT/$t | gzip -c > $OUT/${t}_pass_sequence.txt.gz
  rm -rf $OUT/$t
done
ls -la $OUT
