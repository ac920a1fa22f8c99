#!/usr/bin/env python3
"""The update's optimiser step alone: the fused global-norm clip and Adam step
(hftlob.train.optim.adam_clip_step: hftlob_adam_clip, two launches) against clip_grad_norm_ followed by
capturable torch.optim.Adam.step() (torch's default foreach path), both replayed from a captured HIP
graph, which is how the trainer runs them.

Workload: the parameter tensors of the two ActorCriticRNN nets of 2_player_fq_fqc at H = FC = 256 (14
tensors each), random gradients of global norm 4 (clipped at MAX_GRAD_NORM 0.5), Adam(eps 1e-5, lr 2.5e-4
on the device).  Each path steps its own copy of the net.  Timing is bench_ppo_loss.py's: HIP events on
the launch stream around one graph replay, an untimed clock settle first, then --repeats interleaved
repeats; the medians and ranges are reported.  Before the timing both paths take one step from the same
state and must agree within the tests' bound (per element 1e-5 (|ref| + scale): scale lr for a
parameter, the tensor's mean |ref| for exp_avg and exp_avg_sq, ref the torch path) or the tool fails.

The bytes the operator must move are computed from the sizes: it reads p, g, m, v and writes p, m, v
once (28 bytes per parameter) and reads g a second time for the norm (4 more); over the fused time they
are named as a share of --hbm-gbs (default 8000, the MI355X's 8 TB/s).
Prints one JSON line and writes it to --out (default profiles/adam_clip_bench.json).

    python tools/bench_adam_clip.py [--H 256] [--FC 256] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jaxmarl-hft_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--FC", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_clip_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 9:
        ap.error("--repeats must be at least 9")
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.layout import pack_env_cfg
    from hftlob.train import optim as OP
    from hftlob.train.ippo import ActorCriticRNN

    LR, EPS, MAX_NORM, GRAD_NORM = 2.5e-4, 1e-5, 0.5, 4.0
    cfg = builtin_config("2_player_fq_fqc")
    dims = list(pack_env_cfg(cfg, 10, 100_000, True)[1].obs_dims)
    n_act = [a.n_actions for a in cfg.dict_of_agents_configs.values()]
    names = list(cfg.dict_of_agents_configs)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)

    def make(i, D, A):
        """A net's parameters and their capturable Adam with the state of a first step."""
        torch.manual_seed(i)
        net = ActorCriticRNN(D, A, args.FC, args.H).to(dev)
        params = list(net.parameters())
        opt = torch.optim.Adam(params, lr=torch.tensor(LR, device=dev), eps=EPS, capturable=True)
        OP.init_adam_state(opt)
        return params, opt

    def capture(run):
        side = torch.cuda.Stream(dev)   # warm-up on a side stream (IPPOTrainer._run_step's pattern)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        stream.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        return graph

    def timed(call):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        call()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    def over_bound(got, ref, scale):
        got, ref = got.double(), ref.double()
        return float(((got - ref).abs() / (1e-5 * (ref.abs() + scale))).max())

    calls, sizes, worst = {}, {}, {}
    for i, (name, D, A) in enumerate(zip(names, dims, n_act)):
        (pf, of), (pt, ot) = make(i, D, A), make(i, D, A)
        grads = [torch.randn(p.shape, generator=g, device=dev) for p in pf]
        norm = torch.sqrt(sum((x.double() ** 2).sum() for x in grads))
        grads = [(x * (GRAD_NORM / norm)).float() for x in grads]
        for p, q, x in zip(pf, pt, grads):
            p.grad, q.grad = x.clone(), x.clone()
        sizes[name] = [p.numel() for p in pf]

        def fused(of=of):
            OP.adam_clip_step(of, MAX_NORM)

        def torch_path(pt=pt, ot=ot):
            torch.nn.utils.clip_grad_norm_(pt, MAX_NORM)
            ot.step()

        gf, gt = capture(fused), capture(torch_path)
        # one step of each path from the same state and gradients: they must agree within the tests' bound
        start = [p.detach().clone() for p in pf]
        with torch.no_grad():
            for ps, opt in ((pf, of), (pt, ot)):
                for p, s, x in zip(ps, start, grads):
                    p.copy_(s)
                    p.grad.copy_(x)
                    st = opt.state[p]
                    st["step"].zero_(), st["exp_avg"].zero_(), st["exp_avg_sq"].zero_()
        gf.replay()
        gt.replay()
        torch.cuda.synchronize()
        w = 0.0
        for p, q in zip(pf, pt):
            w = max(w, over_bound(p.detach(), q.detach(), LR))
            for k in ("exp_avg", "exp_avg_sq"):
                ref = ot.state[q][k]
                w = max(w, over_bound(of.state[p][k], ref, float(ref.double().abs().mean())))
            if float(of.state[p]["step"]) != 1.0 or float(ot.state[q]["step"]) != 1.0:
                raise AssertionError(f"{name}: a step counter is not 1 after one step")
        worst[name] = round(w, 4)
        if w > 1.0:
            raise AssertionError(f"{name}: fused and torch differ by {w} of the bound")
        calls[f"fused_{name}"], calls[f"torch_{name}"] = gf.replay, gt.replay

    for c in calls.values():
        timed(c)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    first_torch = next(k for k in calls if k.startswith("torch_"))
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        calls[first_torch]()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.repeats):
        for name, c in calls.items():
            ms[name].append(timed(c))

    med = {k: statistics.median(v) for k, v in ms.items()}
    n_params = {name: sum(s) for name, s in sizes.items()}
    nbytes = {name: 32 * n for name, n in n_params.items()}
    share = lambda b, t_ms: round(b / (t_ms * 1e-3) / (args.hbm_gbs * 1e9), 4)  # noqa: E731
    line = {"tool": "tools/bench_adam_clip.py", "H": args.H, "FC": args.FC, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay, interleaved, median of the repeats",
            "paths": {"fused_*": "adam_clip_step (hftlob_adam_clip: 2 launches), HIP graph",
                      "torch_*": "clip_grad_norm_ + capturable torch.optim.Adam.step() (foreach), HIP graph"},
            "tensors": {name: len(s) for name, s in sizes.items()}, "parameters": n_params,
            "chunks": {name: sum((n + OP.CHUNK - 1) // OP.CHUNK for n in s) for name, s in sizes.items()},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "torch_over_fused": {name: round(med[f"torch_{name}"] / med[f"fused_{name}"], 3) for name in sizes},
            "bytes": nbytes, "hbm_gbs_assumed": args.hbm_gbs,
            "share_of_hbm_bandwidth": {f"fused_{name}": share(nbytes[name], med[f"fused_{name}"]) for name in sizes},
            "max_error_over_bound_fused_vs_torch": worst,
            "device": torch.cuda.get_device_properties(dev).gcnArchName}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
