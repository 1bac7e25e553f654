#!/bin/bash
# GPU parity suite + smoke + short bench (one gpurun call).
# usage: tools/gpu_suite.sh [tag]
set -o pipefail
TAG=${1:-suite}
mkdir -p bench_out
timeout -k 10 840 python -u -m pytest tests -m gpu -x -v --durations=30 --timeout 120 --timeout-method thread > bench_out/pytest_$TAG.log 2>&1
rc=$?; tail -5 bench_out/pytest_$TAG.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > bench_out/smoke_$TAG.log 2>&1 || { cat bench_out/smoke_$TAG.log; exit 1; }
cat bench_out/smoke_$TAG.log
timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --no-cpu > bench_out/bench_$TAG.json 2> bench_out/bench_$TAG.err || { tail bench_out/bench_$TAG.err; exit 1; }
cat bench_out/bench_$TAG.json
