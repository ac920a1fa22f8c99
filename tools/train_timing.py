"""Time the IPPO learner's phases on the GPU (rollout vs PPO epochs) at the metric config.

    python tools/train_timing.py [--graph] [--fused-gru] [--fused-policy] [--fused-loss] [--fused-opt] [--grouped-scan]
                                   [--fused-wgrad] [--fused-wgrad-wide] [--updates N]

--graph: CUDA_GRAPHS (the rollout and each minibatch step replayed as HIP graphs);
--fused-gru: FUSED_GRU (the minibatch step's GRU scan through hftlob_gru_scan_fwd / _bwd);
--fused-policy: FUSED_POLICY (the rollout's policy step, sample and log-prob through hftlob_policy_step);
--fused-loss: FUSED_LOSS (the update's GAE through hftlob_gae, the minibatch step's loss and its gradient through
hftlob_ppo_loss);
--fused-opt: FUSED_OPT (the minibatch step's global-norm clip and Adam step through hftlob_adam_clip);
--grouped-scan: GROUPED_SCAN (the agent types' minibatch steps in lockstep, their scans through
hftlob_gru_scan_fwd_grouped / _bwd_grouped; needs --fused-gru);
--fused-wgrad: FUSED_WGRAD (the narrow layers' weight and bias gradients through hftlob_xty);
--fused-wgrad-wide: FUSED_WGRAD_WIDE (the wide layers' weight and bias gradients through hftlob_xty_wide);
--updates N: the timed rollout + update rounds after the first, untimed update (default 3)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jaxmarl-hft_amd")]

import torch  # noqa: E402

from hftlob.config_io import builtin_config  # noqa: E402
from hftlob.data.synthetic import generate_day  # noqa: E402
from hftlob.env import MARLEnv  # noqa: E402
from hftlob.train import ippo as I  # noqa: E402


def main():
    cfg = builtin_config("2_player_fq_fqc")
    w = cfg.world_config
    day = generate_day(n_msgs=100_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    env = MARLEnv(None, cfg, data=day, return_info=False, persistent_outputs=True)
    graph = "--graph" in sys.argv
    c = I.default_config(NUM_ENVS=4096, NUM_STEPS=64, TOTAL_TIMESTEPS=4096 * 64 * 50, CUDA_GRAPHS=graph,
                         FUSED_GRU="--fused-gru" in sys.argv, FUSED_POLICY="--fused-policy" in sys.argv,
                         FUSED_LOSS="--fused-loss" in sys.argv, FUSED_OPT="--fused-opt" in sys.argv,
                         FUSED_WGRAD="--fused-wgrad" in sys.argv, FUSED_WGRAD_WIDE="--fused-wgrad-wide" in sys.argv,
                         **({"GROUPED_SCAN": True} if "--grouped-scan" in sys.argv else {}))
    rounds = int(sys.argv[sys.argv.index("--updates") + 1]) if "--updates" in sys.argv else 3
    tr = I.IPPOTrainer(env, c)
    tr.update()
    torch.cuda.synchronize()
    for _ in range(rounds):
        t0 = time.perf_counter()
        tr.rollout()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tr.update()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(f"rollout {1e3 * (t1 - t0):.1f} ms  full update (rollout + epochs) {1e3 * (t2 - t1):.1f} ms  "
              f"-> {4096 * 64 / (t2 - t1):.0f} env-steps/s", flush=True)


if __name__ == "__main__":
    main()
