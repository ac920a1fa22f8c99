#!/usr/bin/env python3
"""The learner's GRU sequence scan alone, forward + backward: the fused operators
(hftlob.train.gru.gru_scan: hftlob_gru_scan_fwd / _bwd plus torch's weight-gradient GEMM) against
the loop of ActorCriticRNN.forward (ActorCriticRNN.scan_loop under autograd), both replayed from a
captured HIP graph.

Workload: T = 64, B = 1024, H = 256 (one PPO minibatch of the 4096-env config); random inputs,
done set at 1/64 of the entries.  Each path computes hseq and the gradients of (gi, h0, w_hh, b_hh)
for one fixed cotangent.  Timing is bench_rollout_actions.py's: HIP events on the launch stream,
an untimed clock settle first, then --repeats interleaved repeats of the two graphs; the medians
and spreads are reported.  The two paths' results must agree to the tests' tolerance
(|a - b| <= 1e-5 |b| + 1e-5 max|b| per tensor) or the tool fails.
Prints one JSON line and writes it to --out (default profiles/gru_scan_bench.json).

--groups N times the grouped operators instead (hftlob_gru_scan_fwd_grouped / _bwd_grouped): one launch
of N groups, each a [T, B] batch with its own weights, against N launches of the single-batch operators,
forward and backward separately (the operators alone, without the weight-gradient GEMMs).  The four
graphs are replayed in the same interleaved repeats; the grouped outputs must equal the single ones bit
for bit or the tool fails.  With --out left at its default the line is appended to
profiles/gru_scan_grouped_bench.json (one line per N).

    python tools/bench_gru_scan.py [--T 64] [--B 1024] [--H 256] [--repeats 9] [--groups N]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jaxmarl-hft_amd"))


def grouped_main(args):
    """--groups N: one grouped launch per direction against N single-batch launches."""
    import torch
    from hftlob.train import gru as G

    T, B, H, N = args.T, args.B, args.H, args.groups
    if not G.gru_scan_grouped_supported(H, N):
        raise SystemExit(f"--groups must be in 1..{G.MAX_GROUPS} and --H in {list(G.SUPPORTED_HIDDEN)}")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    xs = [dict(gi=rn(T, B, 3 * H), h0=rn(B, H), done=torch.rand(T, B, generator=g, device=dev) < 1.0 / 64,
               w_hh=rn(3 * H, H) / H ** 0.5, b_hh=0.5 * rn(3 * H), d_hseq=rn(T, B, H)) for _ in range(N)]
    fwd_in = [tuple(x[k] for k in ("gi", "h0", "done", "w_hh", "b_hh")) for x in xs]
    fw0 = [G.scan_forward(*a) for a in fwd_in]   # the backward's inputs (and the warm-up of the forward)
    bwd_in = [(x["d_hseq"], h, gt, x["h0"], x["done"], x["w_hh"]) for x, (h, gt) in zip(xs, fw0)]
    stream = torch.cuda.current_stream(dev)
    runs = {"grouped_fwd": lambda: G.scan_forward_grouped(fwd_in),
            "single_fwd": lambda: [G.scan_forward(*a) for a in fwd_in],
            "grouped_bwd": lambda: G.scan_backward_grouped(bwd_in),
            "single_bwd": lambda: [G.scan_backward(*a) for a in bwd_in]}
    paths = {}
    for name, run in runs.items():
        side = torch.cuda.Stream(dev)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        stream.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        paths[name] = (graph, out)

    def timed(name):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        paths[name][0].replay()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    for name in paths:
        timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        paths["single_fwd"][0].replay()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):
        for name in paths:
            ms[name].append(timed(name))
    for d in ("fwd", "bwd"):
        for k, (a, b) in enumerate(zip(paths["grouped_" + d][1], paths["single_" + d][1])):
            for i, (u, v) in enumerate(zip(a, b)):
                if not torch.equal(u, v):
                    raise AssertionError(f"{d}: group {k}, output {i}: the grouped launch differs from the single one")
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "tools/bench_gru_scan.py --groups", "groups": N, "T": T, "B": B, "H": H, "done_rate": 1.0 / 64,
            "repeats": args.repeats, "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay, interleaved, median of the repeats",
            "paths": {"grouped_fwd": "hftlob_gru_scan_fwd_grouped, one launch of N groups (gates stored)",
                      "single_fwd": "N launches of hftlob_gru_scan_fwd (gates stored)",
                      "grouped_bwd": "hftlob_gru_scan_bwd_grouped, one launch of N groups",
                      "single_bwd": "N launches of hftlob_gru_scan_bwd"},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "single_over_grouped_fwd": round(med["single_fwd"] / med["grouped_fwd"], 3),
            "single_over_grouped_bwd": round(med["single_bwd"] / med["grouped_bwd"], 3),
            "grouped_equals_single_bit_for_bit": True,
            "device": torch.cuda.get_device_properties(dev).gcnArchName}
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", "gru_scan_grouped_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w" if args.out else "a") as f:
        f.write(text + "\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--groups", type=int, default=0, help="time one grouped launch of N groups against N single ones")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 9:
        ap.error("--repeats must be at least 9")
    if args.groups:
        return grouped_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "gru_scan_bench.json")
    import torch
    from hftlob.train.gru import gru_scan
    from hftlob.train.ippo import ActorCriticRNN

    T, B, H = args.T, args.B, args.H
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    done = torch.rand(T, B, generator=g, device=dev) < 1.0 / 64
    d_hseq = rn(T, B, H)
    names = ("gi", "h0", "w_hh", "b_hh")
    x = dict(gi=rn(T, B, 3 * H), h0=rn(B, H), w_hh=rn(3 * H, H) / H ** 0.5, b_hh=0.5 * rn(3 * H))
    stream = torch.cuda.current_stream(dev)

    def capture(scan, backward=True):
        """(graph, hseq, grads) of one forward (+ backward) of `scan` on its own leaves."""
        leaves = {k: v.clone().requires_grad_(backward) for k, v in x.items()}

        def run():
            hseq = scan(leaves["gi"], leaves["h0"], done, leaves["w_hh"], leaves["b_hh"])
            if backward:
                hseq.backward(d_hseq)
            return hseq

        side = torch.cuda.Stream(dev)   # warm-up on a side stream (IPPOTrainer._run_step's pattern)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                for v in leaves.values():
                    v.grad = None
                run()
        stream.wait_stream(side)
        for v in leaves.values():
            v.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hseq = run()
        return graph, hseq.detach(), {k: leaves[k].grad for k in names}

    paths = {"fused": capture(gru_scan), "loop": capture(ActorCriticRNN.scan_loop),
             "fused_fwd": capture(gru_scan, False), "loop_fwd": capture(ActorCriticRNN.scan_loop, False)}

    def timed(name):
        graph = paths[name][0]
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        graph.replay()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    for name in paths:
        timed(name)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        paths["fused"][0].replay()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):
        for name in paths:
            ms[name].append(timed(name))

    worst = {}
    for k, got, ref in [("hseq", paths["fused"][1], paths["loop"][1])] + \
                       [("d_" + n, paths["fused"][2][n], paths["loop"][2][n]) for n in names]:
        got, ref = got.double(), ref.double()
        bound = 1e-5 * ref.abs() + 1e-5 * ref.abs().max()
        worst[k] = round(float(((got - ref).abs() / bound).max()), 4)
        if worst[k] > 1.0:
            raise AssertionError(f"{k}: fused and loop differ by {worst[k]} of the bound")
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "tools/bench_gru_scan.py", "T": T, "B": B, "H": H, "done_rate": 1.0 / 64, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay (forward + backward, or forward only), interleaved, median of the repeats",
            "paths": {"fused": "gru_scan: hftlob_gru_scan_fwd + hftlob_gru_scan_bwd + torch d_w_hh / d_b_hh",
                      "loop": "ActorCriticRNN.scan_loop under autograd",
                      "fused_fwd": "gru_scan, no gradient needed (forward only, gates = NULL)",
                      "loop_fwd": "ActorCriticRNN.scan_loop, no gradient needed (forward only)"},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "loop_over_fused": round(med["loop"] / med["fused"], 3),
            "loop_fwd_over_fused_fwd": round(med["loop_fwd"] / med["fused_fwd"], 3),
            "max_error_over_bound_fused_vs_loop": worst,
            "device": torch.cuda.get_device_properties(dev).gcnArchName}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
