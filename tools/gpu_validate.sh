#!/bin/bash
# On an MI355X: full -m gpu suite, smoke(), the C3 bench with every leg (--full) and the C2 bench;
# logs under $OUT/<tag>_* (OUT defaults to logs/ in the repository root).
# Usage: bash tools/gpu_validate.sh [tag]
TAG=${1:-val}
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-logs}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/${TAG}_gpu_tests.log 2>&1 || exit 1
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || exit 1
timeout -k 10 300 python -u bench.py --full > $OUT/${TAG}_bench_c3.json 2> $OUT/${TAG}_bench_c3.err || exit 1
timeout -k 10 200 python -u bench.py --full --games 256 --blocks 6 --filters 64 --no-cpu-baseline > $OUT/${TAG}_bench_c2.json 2> $OUT/${TAG}_bench_c2.err || exit 1
