#!/usr/bin/env python3
"""The per-episode records of the evaluation launch (MARLEnv.rollout_eval(episodes=):
hftlob_env_rollout_eval_episodes) against the launch without them and against the path a user had
before: per-step outputs and a host-side reduction.

Workload: 2_player_fq_fqc, 4096 envs, T = 256 steps per launch (episodes of 64 or 65 steps: several
episode ends per env), bench.py's synthetic day and reset keys, keys [T, E, 2] (a split_keys chain) and actions
[T, E, action_words] (sample_actions of each step's keys) generated up front.  From one reset state the
tool times, with HIP events on the launch stream,
  eval      env.rollout_eval(stats=): the launch without records
  episodes  env.rollout_eval(stats=, episodes=) with a [E, agents, --cap, 26] buffer
  per_step  env.rollout(per_step=True) followed by hftlob.evaluate.reduce_steps(max_episodes=) over its
            outputs (its launch alone, before the torch reduction, is reported as per_step_launch)
bench.py's practice: an untimed clock settle first, then --repeats interleaved repeats of the chosen
paths, each from the restored reset state; the medians are reported.  The paths' end states must be
equal bit for bit, the statistics of all three equal, and the records of `episodes` equal to those of
`per_step`, or the tool fails.  --paths picks a subset (`eval` alone also runs on a library without the
records' entry points, for a comparison with an earlier build).  Prints one JSON line; --out also
writes it to a file.

    python tools/bench_eval_episodes.py [--envs 4096] [--steps 256] [--cap 4] [--repeats 9]
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
PATHS = ("eval", "episodes", "per_step")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--cap", type=int, default=4, help="records kept per env and agent")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--per-step-repeats", type=int, default=2,
                    help="repeats that also run the per_step path (its reduction is a host loop over the steps)")
    ap.add_argument("--paths", default=",".join(PATHS), help="comma-separated subset of " + ", ".join(PATHS))
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--n-msgs", type=int, default=400_000, help="synthetic day length (bench.py's default)")
    ap.add_argument("--mid", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    paths = [p for p in PATHS if p in args.paths.split(",")]
    if not paths or set(args.paths.split(",")) - set(PATHS):
        ap.error("--paths takes a subset of " + ", ".join(PATHS))
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv, split_keys
    from hftlob.evaluate import reduce_steps

    T, E, cap = args.steps, args.envs, args.cap
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = builtin_config(CONFIG)
    w = cfg.world_config
    day = generate_day(n_msgs=args.n_msgs, mid=args.mid, snap_every=w.n_data_msg_per_step * w.start_resolution)
    # per_step needs the info words, so every path runs on an env that returns them
    env = MARLEnv(None, cfg, data=day, device=dev, return_info=True, persistent_outputs=True)
    params = env.default_params
    all_keys = split_keys(torch.zeros((1, 2), dtype=torch.int32, device=dev), E + 1)[0]
    _, state = env.reset(all_keys[1:].contiguous(), params)
    state0 = state.buf.clone()
    keys = torch.empty((T, E, 2), dtype=torch.int32, device=dev)
    acts = torch.empty((T, E, env.action_words), dtype=torch.int32, device=dev)
    rng = all_keys[1:].contiguous()
    for t in range(T):
        nk = split_keys(rng, 2)
        rng = nk[:, 0].contiguous()
        keys[t] = nk[:, 1]
        acts[t] = env.sample_actions(keys[t])
    stats = {p: torch.zeros((E, env.num_agents, 106), dtype=torch.float64, device=dev) for p in ("eval", "episodes")}
    records = torch.zeros((E, env.num_agents, cap, 26), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    result = {}

    def path_eval():
        stats["eval"].zero_()
        env.rollout_eval(keys, state, acts, params, stats=stats["eval"])
        result["eval"] = (stats["eval"], None)

    def path_episodes():
        stats["episodes"].zero_()
        records.zero_()
        env.rollout_eval(keys, state, acts, params, stats=stats["episodes"], episodes=records)
        result["episodes"] = (stats["episodes"], records)

    def path_per_step():
        _, _, rew, dones, _ = env.rollout(keys, state, acts, params, per_step=True)
        result["launch_done"] = torch.cuda.Event(enable_timing=True)
        result["launch_done"].record(stream)
        result["per_step"] = reduce_steps(rew, env.last_info_words, dones["__all__"], env.layout, max_episodes=cap)

    fns = dict(eval=path_eval, episodes=path_episodes, per_step=path_per_step)
    launch_ms = []

    def timed(name):
        state.buf.copy_(state0)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        fns[name]()
        ev1.record(stream)
        torch.cuda.synchronize()
        if name == "per_step":
            launch_ms.append(ev0.elapsed_time(result["launch_done"]))
        return ev0.elapsed_time(ev1), state.buf.clone()

    def same(a, b):
        return bool(((a == b) | (a.isnan() & b.isnan())).all())

    for name in paths:  # warm-up: module load, output buffers
        if name != "per_step":
            timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        fns[paths[0]]()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for r in range(args.repeats):
        ends = {}
        for name in paths:
            if name == "per_step" and r >= args.per_step_repeats:
                continue
            t_ms, ends[name] = timed(name)
            ms[name].append(t_ms)
        first = next(iter(ends))
        for name in ends:
            if not bool((ends[name] == ends[first]).all()):
                raise AssertionError(f"the end states of {first} and {name} differ")
            if not same(result[name][0], result[first][0]):
                raise AssertionError(f"the statistics of {first} and {name} differ")
        if "episodes" in ends and "per_step" in ends and not same(result["episodes"][1], result["per_step"][1]):
            raise AssertionError("the launch's records differ from reduce_steps over the per-step outputs")
    med = {k: statistics.median(v) for k, v in ms.items() if v}
    line = {"tool": "tools/bench_eval_episodes.py", "config": CONFIG, "envs": E, "steps": T, "cap": cap,
            "repeats": {k: len(v) for k, v in ms.items()}, "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events on the launch stream, median of the interleaved repeats",
            "paths": {"eval": "env.rollout_eval(stats=)", "episodes": "env.rollout_eval(stats=, episodes=)",
                      "per_step": "env.rollout(per_step=True) + evaluate.reduce_steps(max_episodes=)"},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items() if v},
            "env_steps_per_s": {k: round(E * T / (v * 1e-3), 1) for k, v in med.items()},
            "checked_equal": sorted(med), "launch_info": env.launch_info(),
            "device": torch.cuda.get_device_properties(dev).gcnArchName,
            "data": f"synthetic LOBSTER day ({args.n_msgs} msgs, mid {args.mid})"}
    if launch_ms:
        line["per_step_launch_ms"] = round(statistics.median(launch_ms), 4)
    if "episodes" in result:
        line["episodes_per_env"] = float(stats["episodes"][:, 0, 1].mean().item())
    if "eval" in med and "episodes" in med:
        line["episodes_over_eval_ms"] = round(med["episodes"] / med["eval"], 4)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
