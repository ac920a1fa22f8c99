#!/usr/bin/env python3
"""MARLEnv.rollout_eval (hftlob_env_rollout_eval: T tally steps in one persistent launch, rewards
and info words folded into float64 accumulators) against the two ways the same numbers could be
had before it.

Workload: bench.py's (2_player_fq_fqc, 4096 envs, the same synthetic day and reset keys), T = 128
steps per launch, keys [T, E, 2] (a split_keys chain) and actions [T, E, action_words]
(sample_actions of each step's keys) generated up front.  From one reset state the tool times,
with HIP events on the launch stream,
  quiet     (a) env.rollout(per_step=False): the floor (no reward values, no statistics)
  eval      (b) env.rollout_eval
  per_step  (c) env.rollout(per_step=True) followed by hftlob.evaluate.reduce_steps over its
            outputs: what rollout_eval replaces (its launch alone, before the torch reduction, is
            reported beside it as per_step_launch)
bench.py's practice: an untimed clock settle first (back-to-back rollouts for --settle-ms), then
--repeats interleaved repeats of the three, each from the restored reset state; the medians are
reported.  The end states of the three must be equal bit for bit and (b)'s statistics equal to
(c)'s, or the tool fails.  Prints one JSON line and writes the runs and medians to --out (default
profiles/rollout_eval_ab.txt).

    python tools/bench_rollout_eval.py [--envs 4096] [--steps 128] [--repeats 9]
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
PATHS = ("quiet", "eval", "per_step")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--n-msgs", type=int, default=400_000, help="synthetic day length (bench.py's default)")
    ap.add_argument("--mid", type=int, default=2_000_000)
    ap.add_argument("--no-check", action="store_true",
                    help="do not compare the statistics (a knockout build of the library, HFTLOB_LIB=...)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_ab.txt"))
    args = ap.parse_args(argv)
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv, split_keys
    from hftlob.evaluate import reduce_steps

    T, E = args.steps, args.envs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = builtin_config(CONFIG)
    w = cfg.world_config
    day = generate_day(n_msgs=args.n_msgs, mid=args.mid, snap_every=w.n_data_msg_per_step * w.start_resolution)
    # (c) needs the info words, so every path runs on an env that returns them
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
    stats = torch.zeros((E, env.num_agents, 106), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    result = {}

    def path_quiet():
        env.rollout(keys, state, acts, params, per_step=False)

    def path_eval():
        stats.zero_()
        env.rollout_eval(keys, state, acts, params, stats=stats)
        result["eval"] = stats

    def path_per_step():
        _, _, rew, dones, _ = env.rollout(keys, state, acts, params, per_step=True)
        result["launch_done"] = torch.cuda.Event(enable_timing=True)
        result["launch_done"].record(stream)
        result["per_step"] = reduce_steps(rew, env.last_info_words, dones["__all__"], env.layout)

    fns = dict(quiet=path_quiet, eval=path_eval, per_step=path_per_step)

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

    launch_ms = []
    for name in PATHS:  # warm-up: module load, output buffers
        timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        path_quiet()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in PATHS}
    launch_ms = []
    lines = []
    for r in range(args.repeats):
        ends = {}
        for name in PATHS:
            t_ms, ends[name] = timed(name)
            ms[name].append(t_ms)
            lines.append(f"run {r + 1} {name} {E * T / (t_ms * 1e-3):.1f} {t_ms:.4f}")
        if not (bool((ends["quiet"] == ends["eval"]).all()) and bool((ends["quiet"] == ends["per_step"]).all())):
            raise AssertionError("the three paths' end states differ")
        a, b = result["eval"], result["per_step"]
        if not args.no_check and not bool(((a == b) | (a.isnan() & b.isnan())).all()):
            raise AssertionError("rollout_eval's statistics differ from reduce_steps over the per-step outputs")
    med = {k: statistics.median(v) for k, v in ms.items()}
    rate = {k: E * T / (v * 1e-3) for k, v in med.items()}
    line = {"tool": "tools/bench_rollout_eval.py", "config": CONFIG, "envs": E, "steps": T, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events on the launch stream, median of the interleaved repeats",
            "paths": {"quiet": "(a) env.rollout(per_step=False)", "eval": "(b) env.rollout_eval",
                      "per_step": "(c) env.rollout(per_step=True) + evaluate.reduce_steps"},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "env_steps_per_s": {k: round(v, 1) for k, v in rate.items()},
            "per_step_launch": {"ms": round(statistics.median(launch_ms), 4),
                                "env_steps_per_s": round(E * T / (statistics.median(launch_ms) * 1e-3), 1)},
            "eval_over_quiet": round(rate["eval"] / rate["quiet"], 4),
            "eval_over_per_step": round(rate["eval"] / rate["per_step"], 4),
            "end_states_equal": True, "stats_equal": not args.no_check, "launch_info": env.launch_info(),
            "device": torch.cuda.get_device_properties(dev).gcnArchName,
            "data": f"synthetic LOBSTER day ({args.n_msgs} msgs, mid {args.mid})"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"tools/bench_rollout_eval.py on 1x MI355X: {CONFIG}, {E} envs, {T} steps per launch, {args.repeats} "
                "interleaved repeats after the clock settle,\nHIP events; end states and statistics asserted equal.  "
                "Columns: repeat, path, env-steps/s, ms per call.\n"
                "quiet = (a) rollout(per_step=False); eval = (b) rollout_eval; per_step = (c) rollout(per_step=True) + "
                "reduce_steps.\n\n")
        f.write("\n".join(lines) + "\n\n")
        for k in PATHS:
            f.write(f"{k}: median {rate[k] / 1e6:.2f} M env-steps/s ({med[k]:.3f} ms; min {min(ms[k]):.3f} max "
                    f"{max(ms[k]):.3f} ms)\n")
        lm = statistics.median(launch_ms)
        f.write(f"per_step_launch ((c)'s launch alone, before reduce_steps): median {E * T / (lm * 1e-3) / 1e6:.2f} M "
                f"env-steps/s ({lm:.3f} ms)\n")
        f.write(f"eval / quiet {line['eval_over_quiet']}, eval / per_step {line['eval_over_per_step']}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
