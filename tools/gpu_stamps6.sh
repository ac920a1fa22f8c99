#!/bin/bash
# Phase stamps of the quiet step body (ab/stamps_quiet.so) at 1 / 512 / 4096 envs, 20-step launches,
# then the driver's bench command on the in-tree build.  Usage: tools/gpu_stamps6.sh TAG
set -o pipefail
T=${1:-st6}
O=$GRAFT_REPO_ROOT/gpurun_out/$T
mkdir -p $O
cd $GRAFT_REPO_ROOT
for E in 1 512 4096; do
  ST_ENVS=$E ST_STEPS=20 HFTLOB_STAMPS_LIB=ab/stamps_quiet.so timeout -k 10 300 python tools/diag_stamps_rollout.py > $O/stampsq_e$E.txt 2>> $O/stamps.err || exit 1
done
timeout -k 10 300 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench_driver.json 2> $O/bench_driver.err || exit 2
