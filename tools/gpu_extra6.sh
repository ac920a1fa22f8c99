#!/bin/bash
# Round-6 extras on the final kernel: the driver's command under torch.distributed.run (RCCL process
# group, world 1), the 2-rank same-device rehearsal of the N-GPU body (gloo), and the wave-time tail
# statistics at 20 / 128 steps (needs ab/wavetime.so: make -C jaxmarl-hft_amd/csrc wavetime).
# Usage: bash tools/gpu_extra6.sh TAG
set -o pipefail
T=${1:-extra6}
O=$GRAFT_REPO_ROOT/gpurun_out/$T
mkdir -p $O
cd $GRAFT_REPO_ROOT
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 \
  --master-port 29517 bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench_torchrun_rccl.json 2> $O/torchrun.err || exit 1
timeout -k 10 300 python bench.py --gpus 2 --dist-backend gloo --same-device --steps 20 --warmup 5 --no-cpu-baseline > $O/bench_2rank_samedev_gloo.json 2> $O/bench_2rank.err || exit 2
WT_STEPS=20 timeout -k 10 300 python tools/diag_wavetime.py > $O/wavetime_20step.json 2> $O/wavetime.err || exit 3
WT_STEPS=128 timeout -k 10 300 python tools/diag_wavetime.py > $O/wavetime_128step.json 2>> $O/wavetime.err || exit 4
