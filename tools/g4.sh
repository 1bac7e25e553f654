#!/bin/bash
# Coalesced batches (HBM and host) parity, then the batches bench line.
set -o pipefail
mkdir -p bench_out
timeout -k 10 500 python -u -m pytest -x -q --timeout 200 --timeout-method thread tests/test_gpu_batches.py > bench_out/t_g4.log 2>&1
rc=$?; tail -4 bench_out/t_g4.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u bench.py --full --steps 3 --warmup 1 --no-cpu --gather 0 --sweep 0.5 --extra batches > bench_out/b_g4.json 2> bench_out/b_g4.err || { tail bench_out/b_g4.err; exit 1; }
python3 -c "import json; d=json.loads(open('bench_out/b_g4.json').read().strip().splitlines()[-1]); print(json.dumps(d['extra']['batches'], indent=1))"
