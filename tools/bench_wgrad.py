#!/usr/bin/env python3
"""The narrow layers' weight and bias gradients alone: what torch's autograd launches for them
(``d_y.t() @ x`` through rocBLAS and ``d_y.sum(0)``) against the split-over-rows reduction
(hftlob.train.wgrad.xty: hftlob_xty, two launches), both replayed from a captured HIP graph, which is
how the trainer runs them.

Workload: the PPO minibatch of the metric config, N = 64 x 1024 = 65 536 rows, H = FC = 256, and the two
agent types of 2_player_fq_fqc (observation sizes D, action counts A).  The three narrow layers:
    embed    x [N, D],  d_y [N, FC]   d_w [FC, D]   (narrow input:  xty(x, d_y), d_w = C^T, d_b = sum_b)
    actor2   x [N, H],  d_y [N, A]    d_w [A, H]    (narrow output: xty(d_y, x), d_w = C,   d_b = sum_a)
    critic2  x [N, FC], d_y [N, 1]    d_w [1, FC]   (narrow output)
Timing is bench_adam_clip.py's: HIP events on the launch stream around one graph replay, an untimed
clock settle first, then --repeats interleaved rounds; the medians and ranges are reported.  Before the
timing the fused result must agree with float64 on the device within the tests' bound or the tool fails;
both paths' error is reported as a share of that bound.

The bytes a layer's gradient must read are N (P + Q) floats; over a time they are named as a share of
--hbm-gbs (default 6000: the MI355X's measured streaming rate).  --torch-only times the torch pairs
alone (it needs no hftlob_xty in the library).
Prints one JSON line and writes it to --out (default profiles/wgrad_bench.json).

    python tools/bench_wgrad.py [--torch-only] [--N 65536] [--H 256] [--FC 256] [--repeats 9]
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
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--FC", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--hbm-gbs", type=float, default=6000.0)
    ap.add_argument("--torch-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 9:
        ap.error("--repeats must be at least 9")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "wgrad_bench_torch.json" if args.torch_only else "wgrad_bench.json")
    import torch
    from hftlob.config_io import builtin_config
    from hftlob.layout import pack_env_cfg

    cfg = builtin_config("2_player_fq_fqc")
    dims = list(pack_env_cfg(cfg, 10, 100_000, True)[1].obs_dims)
    n_act = [a.n_actions for a in cfg.dict_of_agents_configs.values()]
    names = list(cfg.dict_of_agents_configs)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    N = args.N

    def capture(run):
        side = torch.cuda.Stream(dev)   # warm-up on a side stream (IPPOTrainer._run_step's pattern)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        stream.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        return graph, out

    def timed(call):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        call()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    def over_bound(got, ref):
        got, ref = got.double(), ref.double()
        return float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * ref.abs().max())).max())

    # a captured graph reads its inputs and writes its outputs by address: the tool holds every one of them
    # until the end (torch.cuda.graph empties the allocator's cache on entry, so a tensor released before
    # the next capture is memory a later replay must not touch)
    calls, nbytes, worst, shapes, keep = {}, {}, {}, {}, []
    for name, D, A in zip(names, dims, n_act):
        # (layer, x width, d_y width, narrow input?)
        for layer, wx, wy, narrow_in in (("embed", D, args.FC, True), ("actor2", args.H, A, False),
                                         ("critic2", args.FC, 1, False)):
            key = f"{name}.{layer}"
            x = torch.randn((N, wx), generator=g, device=dev)
            d_y = torch.randn((N, wy), generator=g, device=dev)
            shapes[key] = {"x": [N, wx], "d_y": [N, wy]}
            nbytes[key] = 4 * N * (wx + wy)

            def torch_pair(x=x, d_y=d_y):
                return d_y.t() @ x, d_y.sum(0)

            gt, ref = capture(torch_pair)
            keep.append((x, d_y, gt, ref))
            calls[f"torch_{key}"] = gt.replay
            if args.torch_only:
                continue
            from hftlob.train import wgrad as W

            def fused(x=x, d_y=d_y, narrow_in=narrow_in):
                if narrow_in:
                    c, _, sb = W.xty(x, d_y, want_sum_b=True)
                    return c.t().contiguous(), sb
                c, sa, _ = W.xty(d_y, x, want_sum_a=True)
                return c, sa

            if not W.narrow_linear_supported(wx, wy):
                continue
            gf, got = capture(fused)
            keep.append((gf, got))
            gf.replay()
            gt.replay()
            torch.cuda.synchronize()
            # against float64 on the device, as a share of the tests' bound (both paths)
            r64 = (d_y.double().t() @ x.double(), d_y.double().sum(0))
            worst[key] = {"fused": round(max(over_bound(a, b) for a, b in zip(got, r64)), 4),
                          "torch": round(max(over_bound(a, b) for a, b in zip(ref, r64)), 4)}
            if worst[key]["fused"] > 1.0:
                raise AssertionError(f"{key}: xty differs from float64 by {worst[key]['fused']} of the bound")
            calls[f"fused_{key}"] = gf.replay

    for c in calls.values():
        timed(c)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    first = next(iter(calls))
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        calls[first]()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.repeats):
        for name, c in calls.items():
            ms[name].append(timed(c))

    med = {k: statistics.median(v) for k, v in ms.items()}
    floor_us = {k: round(b / (args.hbm_gbs * 1e9) * 1e6, 2) for k, b in nbytes.items()}
    line = {"tool": "tools/bench_wgrad.py", "N": N, "H": args.H, "FC": args.FC, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay, interleaved, median of the repeats",
            "paths": {"torch_*": "d_y.t() @ x (rocBLAS) and d_y.sum(0), HIP graph",
                      "fused_*": "xty (hftlob_xty: 2 launches; embed with the transpose of C), HIP graph"},
            "shapes": shapes,
            "us": {k: round(1e3 * v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
            "bytes": nbytes, "hbm_gbs_assumed": args.hbm_gbs, "byte_floor_us": floor_us,
            "torch_over_floor": {k: round(1e3 * med[f"torch_{k}"] / floor_us[k], 1) for k in nbytes},
            "device": torch.cuda.get_device_properties(dev).gcnArchName}
    if not args.torch_only:
        line["torch_over_fused"] = {k: round(med[f"torch_{k}"] / med[f"fused_{k}"], 2) for k in nbytes
                                    if f"fused_{k}" in med}
        line["fused_over_floor"] = {k: round(1e3 * med[f"fused_{k}"] / floor_us[k], 1) for k in nbytes
                                    if f"fused_{k}" in med}
        line["max_error_over_bound_vs_float64"] = worst
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
