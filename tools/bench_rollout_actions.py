#!/usr/bin/env python3
"""MARLEnv.rollout (hftlob_env_rollout_actions: T steps with the caller's keys and actions in ONE
persistent launch) against T MARLEnv.step launches over the same inputs.

Workload: bench.py's (2_player_fq_fqc, 4096 envs, the same synthetic day and reset keys), T = 20
and T = 128.  The keys [T, E, 2] (a split_keys chain) and the actions [T, E, action_words]
(sample_actions of each step's keys) are generated up front.  From one reset state the tool times,
with HIP events on the launch stream,
  steps    T env.step launches
  rollout  one env.rollout call
  sampled  one env.rollout_sampled call of T steps as one persistent launch (other keys and
           actions: Speed_test's master-key chain; the same step body, for the near-parity check)
bench.py's practice: an untimed clock settle first (back-to-back rollouts for --settle-ms), then
--repeats interleaved repeats of the three, each from the restored reset state; the medians are
reported.  The end states of `steps` and `rollout` must be equal bit for bit, or the tool fails.
Prints one JSON line and writes it to --out (default profiles/rollout_actions_bench.json).

    python tools/bench_rollout_actions.py [--envs 4096] [--steps 20,128] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jaxmarl-hft_amd"))

CONFIG = "2_player_fq_fqc"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", default="20,128", help="comma-separated rollout lengths T")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--n-msgs", type=int, default=400_000, help="synthetic day length (bench.py's default)")
    ap.add_argument("--mid", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_actions_bench.json"))
    args = ap.parse_args(argv)
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv, split_keys

    lengths = [int(x) for x in args.steps.split(",")]
    Tmax, E = max(lengths), args.envs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = builtin_config(CONFIG)
    w = cfg.world_config
    day = generate_day(n_msgs=args.n_msgs, mid=args.mid, snap_every=w.n_data_msg_per_step * w.start_resolution)
    env = MARLEnv(None, cfg, data=day, device=dev, return_info=False, persistent_outputs=True)
    params = env.default_params
    all_keys = split_keys(torch.zeros((1, 2), dtype=torch.int32, device=dev), E + 1)[0]
    master0 = all_keys[0].clone()
    _, state = env.reset(all_keys[1:].contiguous(), params)
    state0 = state.buf.clone()
    keys = torch.empty((Tmax, E, 2), dtype=torch.int32, device=dev)
    acts = torch.empty((Tmax, E, env.action_words), dtype=torch.int32, device=dev)
    rng = all_keys[1:].contiguous()
    for t in range(Tmax):
        nk = split_keys(rng, 2)
        rng = nk[:, 0].contiguous()
        keys[t] = nk[:, 1]
        acts[t] = env.sample_actions(keys[t])
    kin, kout = master0.clone(), torch.empty_like(master0)
    stream = torch.cuda.current_stream(dev)

    def path_steps(T):
        for t in range(T):
            env.step(keys[t], state, acts[t], params)

    def path_rollout(T):
        env.rollout(keys[:T], state, acts[:T], params)

    def path_sampled(T):
        env.rollout_sampled(kin, kout, state, params, T, n_slices=0)

    def timed(fn, T):
        state.buf.copy_(state0)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        fn(T)
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), state.buf.clone()

    rows = []
    for T in lengths:
        for fn in (path_steps, path_rollout, path_sampled):  # warm-up: module load, output buffers
            timed(fn, T)
        settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
        while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
            path_rollout(T)
            settle_calls += 1
            torch.cuda.synchronize()
        ms = {"steps": [], "rollout": [], "sampled": []}
        for _ in range(args.repeats):
            a, end_steps = timed(path_steps, T)
            b, end_rollout = timed(path_rollout, T)
            c, _ = timed(path_sampled, T)
            ms["steps"].append(a)
            ms["rollout"].append(b)
            ms["sampled"].append(c)
            if not bool((end_steps == end_rollout).all()):
                raise AssertionError(f"T = {T}: env.rollout's end state differs from {T} env.step launches'")
        med = {k: statistics.median(v) for k, v in ms.items()}
        rate = {k: E * T / (v * 1e-3) for k, v in med.items()}
        rows.append({"T": T, "ms": {k: round(v, 4) for k, v in med.items()},
                     "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                     "env_steps_per_s": {k: round(v, 1) for k, v in rate.items()},
                     "rollout_over_steps": round(rate["rollout"] / rate["steps"], 4),
                     "rollout_over_sampled": round(rate["rollout"] / rate["sampled"], 4),
                     "end_states_equal": True, "settle_calls": settle_calls})
    line = {"tool": "tools/bench_rollout_actions.py", "config": CONFIG, "envs": E, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "timing": "HIP events on the launch stream, median of the repeats",
            "paths": {"steps": "T env.step launches (hftlob_env_step)",
                      "rollout": "one env.rollout call (hftlob_env_rollout_actions)",
                      "sampled": "one env.rollout_sampled call, n_slices = 0 (hftlob_env_rollout_sampled)"},
            "launch_info": env.launch_info(), "device": torch.cuda.get_device_properties(dev).gcnArchName,
            "data": f"synthetic LOBSTER day ({args.n_msgs} msgs, mid {args.mid})", "results": rows}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
