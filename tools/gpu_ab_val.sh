#!/bin/bash
# On an MI355X: tests + benches + A/B (base vs new) + rocprof kernel trace of the bench with its legs.
# Logs under $OUT/<tag>_* (OUT: a directory relative to the repository root, default logs).
TAG=${1:-val}
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
export OUT=${OUT:-logs}
mkdir -p $OUT
bash tools/gpu_validate.sh $TAG || exit 1
GAMES=256 BLOCKS=6 FILTERS=64 bash tools/ab_run.sh $OUT/${TAG}_ab_c2.log 800 build_var/base/libaz.so build_var/new/libaz.so || exit 1
bash tools/ab_run.sh $OUT/${TAG}_ab_c3.log 64 build_var/base/libaz.so build_var/new/libaz.so || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/${TAG}_prof -o run -- python3 $R/bench.py --full --steps 1 --warmup 0 --cache 0 --no-cpu-baseline --train-steps 0 > $R/$OUT/${TAG}_prof.log 2>&1 || exit 1
