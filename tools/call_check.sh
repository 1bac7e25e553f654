#!/bin/bash
# Full GPU suite, the per-call probe (phase breakdown), then the batches and
# csv bench lines. usage: tools/call_check.sh <tag>
set -o pipefail
TAG=${1:-call}
mkdir -p bench_out/$TAG
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > bench_out/$TAG/pytest.log 2>&1
rc=$?; tail -4 bench_out/$TAG/pytest.log; [ $rc -ne 0 ] && exit $rc
DFMI_DIAG=1 DFMI_CALL_PROFILE=1 timeout -k 10 120 python tools/call_probe.py > bench_out/$TAG/call_probe.log 2>&1 || { tail bench_out/$TAG/call_probe.log; exit 1; }
grep -v amdgpu.ids bench_out/$TAG/call_probe.log | tail -8
timeout -k 10 400 python bench.py --full --steps 3 --warmup 1 --sweep 0.5 --no-cpu --extra batches,csv > bench_out/$TAG/bench.json 2> bench_out/$TAG/bench.err || { tail bench_out/$TAG/bench.err; exit 1; }
python -c "import json;d=json.loads(open('bench_out/$TAG/bench.json').read().splitlines()[-1]);print(json.dumps(d['extra']))"
