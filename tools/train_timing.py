"""Time the IPPO learner's phases on the GPU (rollout vs PPO epochs) at the metric config.

    python tools/train_timing.py [--graph] [--updates N] [--envs E] [--seed S] [--population P] [--info-dict]
                                 [switch flags]

--graph: CUDA_GRAPHS (the rollout and each minibatch step replayed as HIP graphs);
--updates N: the timed rollout + update rounds after the first, untimed update (default 3);
--envs E: NUM_ENVS (default 4096);
--seed S: SEED (default 2);
--population P: P independent runs (seeds S, S + 1, ...) of E envs each as one hftlob.train.population.PopulationTrainer
instead of one IPPOTrainer; the env-steps/s are those of all the members;
--info-dict: the env built with return_info=True (the info dict of every step) instead of False, or of "raw" under
--train-diag: what the raw mode saves;
the switch flags are the learner's own (hftlob.train.ippo.SWITCHES, but for CALC_EVAL: the evaluation is no part of
the update that is timed):
"""
import argparse
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
from hftlob.train.population import PopulationTrainer  # noqa: E402

TIMED = [sw for sw in I.SWITCHES if sw.key != "CALC_EVAL"]
__doc__ += "".join(f"{sw.flag}: {sw.key} ({sw.help});\n" for sw in TIMED)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--population", type=int, default=0)
    ap.add_argument("--info-dict", action="store_true", help="build the env with return_info=True")
    ap.add_argument("--seed", type=int, default=2, help="SEED of the run (a population's members: seed, seed + 1, ...)")
    for sw in TIMED:
        ap.add_argument(sw.flag, action="store_true")
    a = ap.parse_args()
    cfg = builtin_config("2_player_fq_fqc")
    w = cfg.world_config
    day = generate_day(n_msgs=100_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    info = True if a.info_dict else ("raw" if a.train_diag else False)
    env = MARLEnv(None, cfg, data=day, return_info=info, persistent_outputs=True)
    c = I.default_config(NUM_ENVS=a.envs, NUM_STEPS=64, TOTAL_TIMESTEPS=a.envs * 64 * 50, CUDA_GRAPHS=a.graph, SEED=a.seed,
                         **{sw.key: getattr(a, sw.key.lower()) for sw in TIMED})
    if a.population:
        tr = PopulationTrainer(env, [dict(c, SEED=a.seed + m) for m in range(a.population)])
    else:
        tr = I.IPPOTrainer(env, c)
    steps = a.envs * 64 * max(a.population, 1)
    tr.update()
    torch.cuda.synchronize()
    for _ in range(a.updates):
        t0 = time.perf_counter()
        tr.rollout()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tr.update()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(f"rollout {1e3 * (t1 - t0):.1f} ms  full update (rollout + epochs) {1e3 * (t2 - t1):.1f} ms  "
              f"-> {steps / (t2 - t1):.0f} env-steps/s", flush=True)


if __name__ == "__main__":
    main()
