#!/usr/bin/env python3
"""The wide layers' weight and bias gradients alone: what torch's autograd launches for them
(``d_y.t() @ x`` through rocBLAS and ``d_y.sum(0)``; for the GRU's W_hh the whole of
hftlob.train.gru.weight_grads, with its two concatenations and its select) against the tiled
split-over-rows reduction (hftlob.train.wgrad.xty_wide: hftlob_xty_wide, two launches; for W_hh
hftlob.train.gru.weight_grads_fused), both replayed from a captured HIP graph, which is how the trainer
runs them.

Workload: the PPO minibatch of the metric config, T x B = 64 x 1024 = 65 536 rows, H = FC = 256:
    w_ih     x [N, FC], d_y [N, 3H]      d_w [3H, FC]   xty_wide(d_y, x)
    square   x [N, H],  d_y [N, H]       d_w [H, H]     (actor1, critic1) xty_wide(d_y, x)
    w_hh     d_gi [T, B, 3H], d_gh_n, hseq [T, B, H], h0, done   weight_grads vs weight_grads_fused
Timing is bench_wgrad.py's: HIP events on the launch stream around one graph replay, an untimed clock
settle first, then --repeats interleaved rounds; the medians and ranges are reported, and a shape wins when
the fused path's slowest repeat is below torch's fastest.  Before the timing the fused result must agree
with float64 on the device within the tests' bound or the tool fails; both paths' error is reported as a
share of that bound.  Prints one JSON line and writes it to --out (default profiles/wgrad_wide_bench.json).

    python tools/bench_wgrad_wide.py [--T 64] [--B 1024] [--H 256] [--FC 256] [--repeats 9]
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
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--FC", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgrad_wide_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 9:
        ap.error("--repeats must be at least 9")
    import torch
    from hftlob.train import gru as GR
    from hftlob.train import wgrad as W

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    T, B, H, FC = args.T, args.B, args.H, args.FC
    N = T * B

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

    # (a captured graph reads its inputs and writes its outputs by address: everything is held until the end)
    calls, worst, shapes, flops, keep = {}, {}, {}, {}, []

    def add(key, torch_run, fused_run, ref64):
        gt, ref = capture(torch_run)
        gf, got = capture(fused_run)
        keep.append((gt, ref, gf, got))
        gt.replay()
        gf.replay()
        torch.cuda.synchronize()
        r64 = ref64()
        worst[key] = {"fused": round(max(over_bound(a, b) for a, b in zip(got, r64)), 4),
                      "torch": round(max(over_bound(a, b) for a, b in zip(ref, r64)), 4)}
        if worst[key]["fused"] > 1.0:
            raise AssertionError(f"{key}: xty_wide differs from float64 by {worst[key]['fused']} of the bound")
        calls[f"torch_{key}"], calls[f"fused_{key}"] = gt.replay, gf.replay

    for key, wx, wy in (("w_ih", FC, 3 * H), ("square", H, H)):
        x = torch.randn((N, wx), generator=g, device=dev)
        d_y = torch.randn((N, wy), generator=g, device=dev)
        keep.append((x, d_y))
        shapes[key] = {"x": [N, wx], "d_y": [N, wy]}
        flops[key] = 2 * N * wx * wy
        add(key, lambda x=x, d_y=d_y: (d_y.t() @ x, d_y.sum(0)),
            lambda x=x, d_y=d_y: W.xty_wide([d_y], x, want_sum_a=True),
            lambda x=x, d_y=d_y: (d_y.double().t() @ x.double(), d_y.double().sum(0)))
    d_gi = torch.randn((T, B, 3 * H), generator=g, device=dev)
    d_gh_n = torch.randn((T, B, H), generator=g, device=dev)
    hseq = torch.randn((T, B, H), generator=g, device=dev)
    h0 = torch.randn((B, H), generator=g, device=dev)
    done = torch.rand((T, B), generator=g, device=dev) < 0.1
    keep.append((d_gi, d_gh_n, hseq, h0, done))
    shapes["w_hh"] = {"d_gi": [T, B, 3 * H], "d_gh_n": [T, B, H], "hseq": [T, B, H], "h0": [B, H], "done": [T, B]}
    flops["w_hh"] = 2 * N * H * 3 * H
    add("w_hh", lambda: GR.weight_grads(d_gi, d_gh_n, hseq, h0, done),
        lambda: GR.weight_grads_fused(d_gi, d_gh_n, hseq, h0, done),
        lambda: GR.weight_grads(d_gi.double(), d_gh_n.double(), hseq.double(), h0.double(), done))

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
    line = {"tool": "tools/bench_wgrad_wide.py", "T": T, "B": B, "N": N, "H": H, "FC": FC, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay, interleaved, median of the repeats",
            "paths": {"torch_*": "d_y.t() @ x (rocBLAS) and d_y.sum(0); w_hh: gru.weight_grads (cat, cat, where, "
                                 "GEMM, sum); HIP graph",
                      "fused_*": "xty_wide (hftlob_xty_wide: 2 launches); w_hh: gru.weight_grads_fused; HIP graph"},
            "shapes": shapes,
            "us": {k: round(1e3 * v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
            "tflops": {k: round(flops[k.split("_", 1)[1]] / (1e-3 * v) / 1e12, 1) for k, v in med.items()},
            "torch_over_fused": {k: round(med[f"torch_{k}"] / med[f"fused_{k}"], 2) for k in shapes},
            "fused_wins_by_more_than_the_spread": {k: max(ms[f"fused_{k}"]) < min(ms[f"torch_{k}"]) for k in shapes},
            "max_error_over_bound_vs_float64": worst,
            "device": torch.cuda.get_device_properties(dev).gcnArchName}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
