#!/bin/bash
# Round-6 GPU iteration: the tests named by -k first (new ones), then the whole -m gpu suite (one
# process), then the driver's bench command.  Usage: tools/gpu_r06.sh TAG [pytest -k expr]
set -o pipefail
T=${1:-r06}
O=$GRAFT_REPO_ROOT/gpurun_out/$T
mkdir -p $O
cd $GRAFT_REPO_ROOT
if [ -n "$2" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider -k "$2" > $O/pytest_new.log 2>&1 || exit 1
fi
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider > $O/pytest.log 2>&1 || exit 2
timeout -k 10 300 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench_driver.json 2> $O/bench_driver.err || exit 3
