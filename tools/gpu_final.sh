#!/bin/bash
# On an MI355X, round-end evidence in one call: the full -m gpu suite, smoke(), the C3 bench with
# every leg and the C2 bench (tools/gpu_validate.sh), then the PMC passes over the headline tower
# (tools/pmc_run.sh) and rocprofv3 kernel stats of a plain C3 bench run.  Logs under $OUT/<tag>_*
# (OUT: a directory relative to the repository root, default logs).
# Usage: bash tools/gpu_final.sh <tag>
TAG=${1:-final}
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
export OUT=${OUT:-logs}
mkdir -p $OUT
bash tools/gpu_validate.sh $TAG || exit $?
timeout -k 10 240 bash tools/pmc_run.sh $OUT/${TAG}_pmc_tower32w 2048 8 f32 || exit 5
python3 tools/pmc_summary.py $OUT/${TAG}_pmc_tower32w tower32w_kernel 32 > $OUT/${TAG}_pmc_tower32w_summary.json || exit 6
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/${TAG}_c3prof -o c3 -- \
    python3 $R/bench.py --steps 2 --warmup 1 \
    > $R/$OUT/${TAG}_c3prof.json 2> $R/$OUT/${TAG}_c3prof.err || exit 7
