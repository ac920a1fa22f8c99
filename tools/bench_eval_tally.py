#!/usr/bin/env python3
"""What the tally launch (hftlob_eval_tally, hftlob.evaluate.tally_steps) is worth, measured three ways.

  evaluate   one process run of evaluate_policy: 2_player_fq_fqc, --envs envs x --steps steps, freshly
             initialised nets with H = FC = --hidden (seeded: every run steps the same trajectories),
             greedy.  A short run first (module load, buffers), then the timed run, wall clock from
             the call to its return (EvalStats reads the stats back, so the device is idle at both
             ends).  --pkg names the package tree to import, so the same tool times another checkout
             (its parent commit) through the entry point both have.
  tally      the tally launch alone against evaluate.reduce_steps on the same step outputs: one
             per_step rollout of [--tally-steps, --envs], HIP events on the launch stream, --repeats
             interleaved repeats, the two results asserted equal bit for bit.
  compare    the driver: --runs interleaved `evaluate` child processes per tree (this one and
             --parent-root, a built checkout of the parent commit), then `tally` once, then
             --bench-alternations alternations of each tree's `bench.py --gpus 1`; medians and
             spreads into --out (default profiles/eval_tally_bench.json; an existing file is
             updated, so --runs 0 or --bench-alternations 0 cut a session into calls).  The driver
             itself never opens the GPU: every measurement is a fresh child process.

    python tools/bench_eval_tally.py compare --parent-root /path/to/parent/checkout
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = "2_player_fq_fqc"


def _env_and_nets(args, torch):
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv
    from hftlob.train.ippo import ActorCriticRNN
    cfg = builtin_config(CONFIG)
    w = cfg.world_config
    day = generate_day(n_msgs=args.n_msgs, snap_every=w.n_data_msg_per_step * w.start_resolution)
    env = MARLEnv(None, cfg, data=day, device="cuda:0", return_info=True, persistent_outputs=True)
    torch.manual_seed(0)
    nets = [ActorCriticRNN(env.observation_spaces[i].shape[0], env.action_spaces[i].n, args.hidden, args.hidden).cuda()
            for i in range(len(env.action_spaces))]
    return env, nets


def run_evaluate(args):
    sys.path.insert(0, args.pkg)
    import torch
    import hftlob
    from hftlob.evaluate import evaluate_policy
    env, nets = _env_and_nets(args, torch)
    evaluate_policy(env, nets, args.envs, 8, 0, greedy=True)            # module load, output buffers
    torch.cuda.synchronize()
    secs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        ev = evaluate_policy(env, nets, args.envs, args.steps, 1, greedy=True)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    print(json.dumps({"mode": "evaluate", "package": os.path.dirname(os.path.abspath(hftlob.__file__)),
                      "envs": args.envs, "steps": args.steps, "hidden": args.hidden, "seconds": [round(s, 5) for s in secs],
                      "avg_reward": [ev.reward(t)["mean"] for t in range(len(nets))], "total_dones": ev.total_dones()}))
    return 0


def run_tally(args):
    sys.path.insert(0, args.pkg)
    import torch
    from hftlob.env import split_keys
    from hftlob.evaluate import reduce_steps, tally_steps
    env, _ = _env_and_nets(args, torch)
    T, E, dev = args.tally_steps, args.envs, torch.device("cuda", 0)
    params = env.default_params
    all_keys = split_keys(torch.zeros((1, 2), dtype=torch.int32, device=dev), E + 1)[0]
    _, state = env.reset(all_keys[1:].contiguous(), params)
    keys = split_keys(all_keys[1:].contiguous(), T).transpose(0, 1).contiguous()      # [T, E, 2]
    acts = torch.stack([env.sample_actions(keys[t]) for t in range(T)])
    _, _, rew, dones, _ = env.rollout(keys, state, acts, params, per_step=True)
    rew = torch.cat([x.reshape(T, E, -1) for x in rew], dim=2).contiguous()
    info, done = env.last_info_words.reshape(T, E, -1).clone(), dones["__all__"].clone()
    stream = torch.cuda.current_stream(dev)
    stats = torch.zeros((E, rew.shape[2], 106), dtype=torch.float64, device=dev)
    out = {}

    def path_reduce():
        out["reduce_steps"] = reduce_steps(rew, info, done, env.layout)

    def path_tally():
        stats.zero_()
        out["tally_steps"] = tally_steps(rew, info, done, env.layout, stats)

    fns = {"reduce_steps": path_reduce, "tally_steps": path_tally}

    def timed(name):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        fns[name]()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    for name in fns:
        timed(name)
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):
        for name in fns:
            ms[name].append(timed(name))
        a, b = out["reduce_steps"], out["tally_steps"]
        if not bool(((a == b) | (a.isnan() & b.isnan())).all()):
            raise AssertionError("tally_steps differs from reduce_steps")
    print(json.dumps({"mode": "tally", "envs": E, "steps": T, "repeats": args.repeats,
                      "timing": "HIP events on the launch stream (tally_steps includes zeroing its stats)",
                      "ms_median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                      "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                      "equal": True, "device": torch.cuda.get_device_properties(dev).gcnArchName}))
    return 0


def _child(cmd, cwd, timeout):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _spread(v):
    return {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v)}


def run_compare(args):
    trees = {"parent": os.path.abspath(args.parent_root), "new": ROOT}
    me = os.path.abspath(__file__)
    common = ["--envs", str(args.envs), "--steps", str(args.steps), "--hidden", str(args.hidden),
              "--n-msgs", str(args.n_msgs)]
    result = {}
    if os.path.exists(args.out):   # a session may be cut into calls (--runs 0 / --bench-alternations 0): they add up
        with open(args.out) as f:
            result = json.load(f)
    result.update({"tool": "tools/bench_eval_tally.py", "config": CONFIG, "envs": args.envs, "steps": args.steps,
                   "hidden": args.hidden, "n_msgs": args.n_msgs})
    secs = {k: [] for k in trees}
    check = {}
    for r in range(args.runs):
        for name, root in trees.items():
            rec = _child([sys.executable, me, "evaluate", "--pkg", os.path.join(root, "jaxmarl-hft_amd"), "--repeats", "1"]
                         + common, root, 600)
            secs[name].append(rec["seconds"][0])
            check.setdefault(name, (rec["avg_reward"], rec["total_dones"]))
            print(f"evaluate run {r + 1} {name}: {rec['seconds'][0]:.4f} s", flush=True)
    if args.runs:
        if json.dumps(check["parent"]) != json.dumps(check["new"]):
            raise AssertionError(f"the two trees' evaluations differ: {check}")
        result["evaluate_policy"] = {"what": "wall seconds of one evaluate_policy call per process run, the trees "
                                             "interleaved", "results_equal": True, "avg_reward": check["new"][0],
                                     **{k: _spread(v) for k, v in secs.items()}}
        result["evaluate_policy"]["new_over_parent"] = round(statistics.median(secs["new"])
                                                             / statistics.median(secs["parent"]), 4)
        result["tally_alone"] = _child([sys.executable, me, "tally", "--pkg", os.path.join(ROOT, "jaxmarl-hft_amd"),
                                        "--repeats", str(args.repeats), "--tally-steps", str(args.tally_steps)] + common,
                                       ROOT, 600)
        print("tally alone:", json.dumps(result["tally_alone"]["ms_median"]), flush=True)
    rates = {k: [] for k in trees}
    for r in range(args.bench_alternations):
        for name, root in trees.items():
            rec = _child([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps),
                          "--warmup", str(args.bench_warmup)], root, 900)
            rates[name].append(rec["value"])
            print(f"bench.py alternation {r + 1} {name}: {rec['value']}", flush=True)
    if args.bench_alternations:
        result["bench_py"] = {"what": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}, its "
                                      "'value', the trees alternated", **{k: _spread(v) for k, v in rates.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("evaluate_policy", "tally_alone") if k in result}))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("evaluate", "tally", "compare"))
    ap.add_argument("--pkg", default=os.path.join(ROOT, "jaxmarl-hft_amd"), help="the package tree to import")
    ap.add_argument("--parent-root", default=None, help="compare: a built checkout of the parent commit")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=256, help="GRU_HIDDEN_DIM = FC_DIM_SIZE of the nets")
    ap.add_argument("--tally-steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9, help="timed repeats inside an evaluate / tally process")
    ap.add_argument("--runs", type=int, default=5, help="compare: evaluate process runs per tree")
    ap.add_argument("--bench-alternations", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=128)
    ap.add_argument("--bench-warmup", type=int, default=16)
    ap.add_argument("--n-msgs", type=int, default=400_000, help="synthetic day length (bench.py's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_tally_bench.json"))
    args = ap.parse_args(argv)
    if args.mode == "compare" and not args.parent_root:
        ap.error("compare needs --parent-root")
    return {"evaluate": run_evaluate, "tally": run_tally, "compare": run_compare}[args.mode](args)


if __name__ == "__main__":
    sys.exit(main())
