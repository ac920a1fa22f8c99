#!/usr/bin/env python3
"""MARLEnv.rollout_eval_drawn (hftlob_env_rollout_eval_drawn: a uniform baseline policy's actions drawn
inside the persistent evaluation launch) against the launches it stands next to.

Workload: tools/bench_rollout_eval.py's (2_player_fq_fqc, 4096 envs, the same synthetic day and reset
keys), T = 256 steps per launch, keys [T, E, 2] and draw keys [T, n_types, 2] generated up front,
Uniform.all() for both agent types.  From one reset state the tool times, with HIP events on the launch
stream,
  drawn     env.rollout_eval_drawn
  fixed     (a) env.rollout_eval(fixed=True) on the same keys with one fixed action per type: the
            launch without a draw (its envs take another trajectory, so the difference also holds
            what the random actions do to the books)
  replay    env.rollout_eval fed the [T, E, action_words] actions the drawn launch wrote: the same
            trajectory with the actions read instead of drawn, so drawn - replay is the draw alone
  per_step  (b) per step one hftlob_draw_actions launch per type, env.step and the tally launch:
            evaluate_policy's loop for the same entries
bench.py's practice: an untimed clock settle first, then --repeats interleaved repeats of the four,
each from the restored reset state; medians and min / max are reported.  drawn's end state and
statistics must equal replay's and per_step's bit for bit, or the tool fails.  Prints one JSON line
and writes it with the runs to --out (default profiles/eval_drawn_bench.json).

    python tools/bench_eval_drawn.py [--envs 4096] [--steps 256] [--repeats 9]
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
PATHS = ("drawn", "fixed", "replay", "per_step")
FIXED = [4, 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--n-msgs", type=int, default=400_000, help="synthetic day length (bench.py's default)")
    ap.add_argument("--mid", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_drawn_bench.json"))
    args = ap.parse_args(argv)
    import torch
    from hftlob import evaluate as EV
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv, split_keys

    T, E = args.steps, args.envs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = builtin_config(CONFIG)
    w = cfg.world_config
    day = generate_day(n_msgs=args.n_msgs, mid=args.mid, snap_every=w.n_data_msg_per_step * w.start_resolution)
    # per_step tallies from the info words, so every path runs on an env that returns them
    env = MARLEnv(None, cfg, data=day, device=dev, return_info=True, persistent_outputs=True)
    params, L = env.default_params, env.layout
    counts = list(cfg.number_of_agents_per_type)
    sizes = [sp.n for sp in env.action_spaces]
    masks = [EV.Uniform.all().mask(n) for n in sizes]
    all_keys = split_keys(torch.zeros((1, 2), dtype=torch.int32, device=dev), E + 1)[0]
    _, state = env.reset(all_keys[1:].contiguous(), params)
    state0 = state.buf.clone()
    keys = torch.empty((T, E, 2), dtype=torch.int32, device=dev)
    rng = all_keys[1:].contiguous()
    for t in range(T):
        nk = split_keys(rng, 2)
        rng = nk[:, 0].contiguous()
        keys[t] = nk[:, 1]
    dk = split_keys(all_keys[:1].contiguous(), T * len(counts)).view(T, len(counts), 2).contiguous()
    row = EV.fixed_action_row(env, FIXED)
    A = env.num_agents
    stats = {k: torch.zeros((E, A, 106), dtype=torch.float64, device=dev) for k in PATHS}
    acts = torch.zeros((T, E, env.action_words), dtype=torch.int32, device=dev)
    step_acts = [torch.empty((E, n), dtype=torch.int32, device=dev) for n in counts]
    fw = EV._float_word_masks(L)
    stream = torch.cuda.current_stream(dev)

    def path_drawn():
        env.rollout_eval_drawn(keys, state, dk, masks, params, stats=stats["drawn"], actions_out=acts)

    def path_fixed():
        env.rollout_eval(keys, state, row, params, stats=stats["fixed"], fixed=True)

    def path_replay():  # (reads what the last drawn call wrote: the same inputs give the same actions every repeat)
        env.rollout_eval(keys, state, acts, params, stats=stats["replay"])

    def path_per_step():
        st = stats["per_step"]
        for t in range(T):
            for i, n in enumerate(counts):
                EV._draw_launch(E * n, sizes[i], masks[i], dk[t, i], step_acts[i])
            _, _, _, d, _ = env.step(keys[t], state, step_acts, params)
            EV._tally_launch(env.last_rewards.view(1, E, A), env.last_info_words.view(1, E, L.info_words),
                             d["__all__"].view(torch.uint8).view(1, E), fw, L.info_words, st)

    fns = dict(drawn=path_drawn, fixed=path_fixed, replay=path_replay, per_step=path_per_step)

    def timed(name):
        state.buf.copy_(state0)
        stats[name].zero_()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        fns[name]()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), state.buf.clone()

    for name in PATHS:  # warm-up: module load, output buffers (drawn first: replay reads its actions)
        timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        path_fixed()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in PATHS}
    runs = []
    for r in range(args.repeats):
        ends = {}
        for name in PATHS:
            t_ms, ends[name] = timed(name)
            ms[name].append(t_ms)
            runs.append({"repeat": r + 1, "path": name, "ms": round(t_ms, 4),
                         "env_steps_per_s": round(E * T / (t_ms * 1e-3), 1)})
        for other in ("replay", "per_step"):
            if not bool((ends["drawn"] == ends[other]).all()):
                raise AssertionError(f"the end states of drawn and {other} differ")
            a, b = stats["drawn"], stats[other]
            if not bool(((a == b) | (a.isnan() & b.isnan())).all()):
                raise AssertionError(f"the statistics of drawn and {other} differ")
    med = {k: statistics.median(v) for k, v in ms.items()}
    rate = {k: E * T / (v * 1e-3) for k, v in med.items()}
    line = {"tool": "tools/bench_eval_drawn.py", "config": CONFIG, "envs": E, "steps": T, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events on the launch stream, median of the interleaved repeats",
            "paths": {"drawn": "env.rollout_eval_drawn, Uniform.all() for both types",
                      "fixed": f"(a) env.rollout_eval(fixed=True), actions {FIXED}",
                      "replay": "env.rollout_eval fed the drawn launch's actions_out",
                      "per_step": "(b) hftlob_draw_actions per type + env.step + hftlob_eval_tally, per step"},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "env_steps_per_s": {k: round(v, 1) for k, v in rate.items()},
            "drawn_over_fixed_ms": round(med["drawn"] / med["fixed"], 4),
            "drawn_over_replay_ms": round(med["drawn"] / med["replay"], 4),
            "per_step_over_drawn_ms": round(med["per_step"] / med["drawn"], 4),
            "draw_ns_per_env_step": round((med["drawn"] - med["replay"]) * 1e6 / (E * T), 3),
            "end_states_equal": True, "stats_equal": True, "n_actions": sizes, "launch_info": env.launch_info(),
            "device": torch.cuda.get_device_properties(dev).gcnArchName,
            "data": f"synthetic LOBSTER day ({args.n_msgs} msgs, mid {args.mid})"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"result": line, "runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
