#!/usr/bin/env python3
"""The rollout's per-step policy work alone, for each agent type of 2_player_fq_fqc: the fused
operator (hftlob.train.policy.policy_step, mode 0: one hftlob_policy_step launch that updates the
carry in place and writes action, log-prob and value into the rollout buffers' rows) against today's
path exactly as IPPOTrainer._rollout runs it (net.step + softmax + multinomial + log_softmax / gather
+ the carry copy and the three buffer copies), both replayed from a captured HIP graph.

Workload: B = 4096 actors, H = FC = 256, D and A of the agent type; random inputs, done at 1/64 of
the rows.  Timing is bench_gru_scan.py's: HIP events on the launch stream around one graph replay, an
untimed clock settle first, then --repeats interleaved repeats of the graphs; medians and spreads are
reported.  The fused h, value and log-prob (at the fused action) must agree with net.step on the same
inputs to the tests' tolerance (|a - b| <= 1e-5 |b| + 1e-5 max|b| per tensor) or the tool fails.
The measurement runs in a child process under a time limit; the parent only waits for it.
Prints one JSON line and writes it to --out (default profiles/policy_step_bench.json).

    python tools/bench_policy_step.py [--B 4096] [--H 256] [--FC 256] [--repeats 9] [--timeout 240]

With --groups G --batch B the tool measures the grouped operator instead: G nets (the config's agent types in
turn, each with its own weights, B actors each) stepped by G separate policy_step_net launches against ONE
policy_step_grouped launch, both replayed from a captured HIP graph, timed as above.  The two paths' outputs
must agree bit for bit or the tool fails.  One JSON line is printed and appended to --out (default
profiles/policy_step_grouped_bench.json).

    python tools/bench_policy_step.py --groups 8 --batch 1024 [--H 256] [--FC 256] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jaxmarl-hft_amd"))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--FC", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--groups", type=int, default=0, help="G > 0: G separate launches against one grouped launch")
    ap.add_argument("--batch", type=int, default=1024, help="with --groups: the actors of each group")
    ap.add_argument("--out", default=None, help="default profiles/policy_step_bench.json, with --groups "
                    "profiles/policy_step_grouped_bench.json (appended to)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap


def worker(args):
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.layout import pack_env_cfg
    from hftlob.train.ippo import ActorCriticRNN
    from hftlob.train.policy import SAMPLE, policy_step

    cfg = builtin_config("2_player_fq_fqc")
    dims = list(pack_env_cfg(cfg, 10, 100_000, True)[1].obs_dims)
    n_act = [a.n_actions for a in cfg.dict_of_agents_configs.values()]
    names = list(cfg.dict_of_agents_configs)
    B, H, FC = args.B, args.H, args.FC
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)   # multinomial's generator, as the trainer's

    def capture(run, register=None):
        side = torch.cuda.Stream(dev)   # warm-up on a side stream (IPPOTrainer's pattern)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        stream.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        if register is not None:
            graph.register_generator_state(register)
        with torch.cuda.graph(graph):
            run()
        return graph

    paths, checks = {}, {}
    for i, (name, D, A) in enumerate(zip(names, dims, n_act)):
        torch.manual_seed(i)
        net = ActorCriticRNN(D, A, FC, H).to(dev)
        with torch.no_grad():   # a head with a real logit range (the initialiser's 0.01 gain is near uniform)
            net.actor2.weight.mul_(100.0)
        obs = torch.randn(B, D, generator=g, device=dev)
        done = torch.rand(B, generator=g, device=dev) < 1.0 / 64
        h0 = torch.randn(B, H, generator=g, device=dev)
        key = torch.tensor([0, 7 + i], dtype=torch.int32, device=dev)
        hf, ht = h0.clone(), h0.clone()
        mk = lambda: (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev),  # noqa: E731
                      torch.empty(B, device=dev))
        (af, lf, vf), (at, lt, vt) = mk(), mk()

        def fused(net=net, obs=obs, done=done, hf=hf, key=key, out=(af, lf, vf)):
            policy_step(net, obs, done, hf, SAMPLE, key=key, out=out)

        def today(net=net, obs=obs, done=done, ht=ht, at=at, lt=lt, vt=vt):
            h, logits, v = net.step(ht, obs, done)
            ht.copy_(h)
            probs = torch.softmax(logits, -1)
            a = torch.multinomial(probs, 1, generator=gen).squeeze(-1)
            at.copy_(a)
            vt.copy_(v)
            lt.copy_(torch.log_softmax(logits, -1).gather(-1, a.unsqueeze(-1)).squeeze(-1))

        with torch.no_grad():
            # agreement on the same inputs (one step from h0), before the graphs start moving the carries
            h1, logits, v1 = net.step(h0, obs, done)
            fused()
            torch.cuda.synchronize()
            lp = torch.log_softmax(logits.double(), -1).gather(-1, af.long()[:, None]).squeeze(-1)
            worst = {}
            for k, got, ref in (("h", hf, h1), ("value", vf, v1), ("log_prob", lf, lp)):
                got, ref = got.double(), ref.double()
                bound = 1e-5 * ref.abs() + 1e-5 * ref.abs().max()
                worst[k] = round(float(((got - ref).abs() / bound).max()), 4)
                if worst[k] > 1.0:
                    raise AssertionError(f"{name} {k}: fused and net.step differ by {worst[k]} of the bound")
            checks[name] = worst
            paths[f"fused_{name}"] = capture(fused)
            paths[f"today_{name}"] = capture(today, register=gen)

    def timed(name):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        paths[name].replay()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    for name in paths:
        timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    first = next(iter(paths))
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        paths[first].replay()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):
        for name in paths:
            ms[name].append(timed(name))
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "tools/bench_policy_step.py", "B": B, "H": H, "FC": FC, "env_config": "2_player_fq_fqc",
            "types": {n: {"D": d, "A": a} for n, d, a in zip(names, dims, n_act)}, "done_rate": 1.0 / 64,
            "repeats": args.repeats, "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay, interleaved, median of the repeats",
            "paths": {"fused": "policy_step mode 0: one hftlob_policy_step launch (carry in place, outputs into the buffers)",
                      "today": "net.step + softmax + multinomial + log_softmax / gather + the carry and buffer copies"},
            "us": {k: round(1e3 * v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
            "today_over_fused": {n: round(med[f"today_{n}"] / med[f"fused_{n}"], 3) for n in names},
            "max_error_over_bound_fused_vs_net_step": checks,
            "device": torch.cuda.get_device_properties(dev).gcnArchName}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


def worker_groups(args):
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.layout import pack_env_cfg
    from hftlob.train.ippo import ActorCriticRNN
    from hftlob.train.policy import MAX_GROUPS, SAMPLE, policy_step_grouped, policy_step_net

    cfg = builtin_config("2_player_fq_fqc")
    dims = list(pack_env_cfg(cfg, 10, 100_000, True)[1].obs_dims)
    n_act = [a.n_actions for a in cfg.dict_of_agents_configs.values()]
    G, B, H, FC = args.groups, args.batch, args.H, args.FC
    if not 1 <= G <= MAX_GROUPS:
        raise SystemExit(f"--groups must be in 1..{MAX_GROUPS}")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    nets, obss, dones, h0s, keys = [], [], [], [], []
    for k in range(G):
        D, A = dims[k % len(dims)], n_act[k % len(dims)]
        torch.manual_seed(k)
        net = ActorCriticRNN(D, A, FC, H).to(dev)
        with torch.no_grad():
            net.actor2.weight.mul_(100.0)
        nets.append(net)
        obss.append(torch.randn(B, D, generator=g, device=dev))
        dones.append(torch.rand(B, generator=g, device=dev) < 1.0 / 64)
        h0s.append(torch.randn(B, H, generator=g, device=dev))
        keys.append(torch.tensor([0, 7 + k], dtype=torch.int32, device=dev))
    mk = lambda: [(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev),  # noqa: E731
                   torch.empty(B, device=dev)) for _ in range(G)]
    hs, hg, outs_s, outs_g = [h.clone() for h in h0s], [h.clone() for h in h0s], mk(), mk()

    def separate():
        for k in range(G):
            policy_step_net(nets[k], obss[k], dones[k], hs[k], SAMPLE, key=keys[k], out=outs_s[k])

    def grouped():
        policy_step_grouped(nets, obss, dones, hg, SAMPLE, keys=keys, outs=outs_g)

    def capture(run):
        side = torch.cuda.Stream(dev)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        stream.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        return graph

    with torch.no_grad():
        separate()
        grouped()
        torch.cuda.synchronize()
        for k in range(G):   # the same step from the same carry: the two paths agree bit for bit
            if not (torch.equal(hs[k], hg[k]) and all(torch.equal(a, b) for a, b in zip(outs_s[k], outs_g[k]))):
                raise AssertionError(f"group {k}: the grouped launch differs from the separate one")
        paths = {"separate": capture(separate), "grouped": capture(grouped)}

    def timed(name):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        paths[name].replay()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    for name in paths:
        timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        paths["separate"].replay()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):
        for name in paths:
            ms[name].append(timed(name))
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "tools/bench_policy_step.py --groups", "groups": G, "batch": B, "H": H, "FC": FC,
            "env_config": "2_player_fq_fqc", "tiles": G * ((B + 15) // 16), "done_rate": 1.0 / 64,
            "repeats": args.repeats, "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay, interleaved, median of the repeats",
            "paths": {"separate": "G policy_step_net launches (mode 0), one per net",
                      "grouped": "one policy_step_grouped launch (mode 0) of the G nets"},
            "us": {k: round(1e3 * v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
            "separate_over_grouped": round(med["separate"] / med["grouped"], 3),
            "bit_equal": True, "device": torch.cuda.get_device_properties(dev).gcnArchName}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
    return 0


def main(argv=None):
    args = parser().parse_args(argv)
    if args.repeats < 9:
        parser().error("--repeats must be at least 9")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "policy_step_grouped_bench.json" if args.groups
                                else "policy_step_bench.json")
    if args.worker:
        return worker_groups(args) if args.groups else worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + list(sys.argv[1:] if argv is None else argv)
    try:   # the GPU work in a fresh child under its own time limit
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"bench_policy_step: the measuring process exceeded {args.timeout} s and was stopped", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
