#!/usr/bin/env python3
"""The update's objective alone: the fused PPO loss with its gradient (hftlob.train.loss.ppo_loss_fused:
hftlob_ppo_loss, three launches) against ppo_loss_multi plus backward, both replayed from a captured
HIP graph; and the fused GAE (hftlob.train.loss.gae, one launch) against the loop of calculate_gae,
both eager, which is how the trainer runs them.

Workload: the loss at N = 64 x 1024 elements (one PPO minibatch of the 4096-env config) for
nvec = [10] and [13], the two agent types of 2_player_fq_fqc; GAE at T = 64, n = 4096.  Random inputs
(adv = 3 randn + 1, rb_log_prob = the policy's log-prob + 0.2 randn, rb_value = values + 0.3 randn).
Timing is bench_gru_scan.py's: HIP events on the launch stream, an untimed clock settle first, then
--repeats interleaved repeats; the medians and spreads are reported.  The fused loss and the torch
loss must agree to the tests' tolerance or the tool fails; GAE must agree bit for bit.

The bytes the loss operator must move are computed from the shapes: it reads logits [N, S], actions
[N, K] and five [N] vectors (adv a second time for its moments) and writes d_logits [N, S] and d_values
[N]; over the fused time they are named as a share of --hbm-gbs (default 8000, the MI355X's 8 TB/s).
GAE reads reward, value [T, n], done bytes and writes adv, targets.
Prints one JSON line and writes it to --out (default profiles/ppo_loss_bench.json).

    python tools/bench_ppo_loss.py [--T 64] [--B 1024] [--n 4096] [--repeats 9]
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
    ap.add_argument("--n", type=int, default=4096, help="actors of the GAE workload")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_loss_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 9:
        ap.error("--repeats must be at least 9")
    import torch
    from hftlob.train import loss as LS
    from hftlob.train.ippo import calculate_gae, ppo_loss_multi

    T, B = args.T, args.B
    N = T * B
    EPS, VF, ENT = 0.2, 0.5, 0.01
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    stream = torch.cuda.current_stream(dev)

    def loss_inputs(nvec):
        logits, values = 2.0 * rn(T, B, sum(nvec)), rn(T, B)
        actions = torch.stack([torch.randint(0, n, (T, B), generator=g, device=dev) for n in nvec], -1).to(torch.int32)
        lp = sum(torch.log_softmax(x, -1).gather(-1, actions[..., k].long().unsqueeze(-1)).squeeze(-1)
                 for k, x in enumerate(logits.split(nvec, -1)))
        return [logits, values, actions, values + 0.3 * rn(T, B), lp + 0.2 * rn(T, B), 3.0 * rn(T, B) + 1.0, rn(T, B)]

    def capture(fn, x, nvec):
        """(graph, the six scalars, d_logits, d_values) of one loss + backward of `fn` on its own leaves."""
        lg, v = x[0].clone().requires_grad_(True), x[1].clone().requires_grad_(True)

        def run():
            out = fn(lg, v, *x[2:], EPS, VF, ENT, nvec)
            out[0].backward()
            return torch.stack([t.detach() for t in out])

        side = torch.cuda.Stream(dev)   # warm-up on a side stream (IPPOTrainer._run_step's pattern)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for _ in range(2):
                lg.grad = v.grad = None
                run()
        stream.wait_stream(side)
        lg.grad = v.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            stats = run()
        return graph, stats, lg, v

    def timed(call):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        call()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    heads = {"10": [10], "13": [13]}
    paths, inputs = {}, {}
    for tag, nvec in heads.items():
        inputs[tag] = loss_inputs(nvec)
        paths[f"fused_{tag}"] = capture(LS.ppo_loss_fused, inputs[tag], nvec)
        paths[f"torch_{tag}"] = capture(ppo_loss_multi, inputs[tag], nvec)
    calls = {k: p[0].replay for k, p in paths.items()}

    n = args.n
    gx = (rn(T, n), rn(T, n), torch.rand(T, n, generator=g, device=dev) < 1.0 / 64, rn(n))
    GAMMA, LAM = 0.999, 0.9
    gae_out = {}
    calls["gae_fused"] = lambda: gae_out.__setitem__("fused", LS.gae(*gx, GAMMA, LAM))
    calls["gae_loop"] = lambda: gae_out.__setitem__("loop", calculate_gae(*gx, GAMMA, LAM))

    for c in calls.values():
        timed(c)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        calls["torch_10"]()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.repeats):
        for name, c in calls.items():
            ms[name].append(timed(c))

    worst = {}
    for tag in heads:
        f, t = paths[f"fused_{tag}"], paths[f"torch_{tag}"]
        for k, got, ref in (("d_logits", f[2].grad, t[2].grad), ("d_values", f[3].grad, t[3].grad)):
            got, ref = got.double(), ref.double()
            bound = 1e-5 * ref.abs() + 1e-5 * ref.abs().max()
            worst[f"{k}_{tag}"] = round(float(((got - ref).abs() / bound).max()), 4)
        m = [float(x.abs().mean()) for x in LS.ppo_loss_elements(*[a.double() if a.is_floating_point() else a
                                                                     for a in inputs[tag]], EPS, heads[tag])["terms"]]
        m = [m[1] + VF * 0.5 * m[0] + ENT * m[2], 0.5 * m[0], m[1], m[2], m[3], m[4]]
        err = (f[1].double() - t[1].double()).abs() / (1e-5 * (t[1].double().abs() + torch.tensor(m, device=dev)))
        worst[f"scalars_{tag}"] = round(float(err.max()), 4)
    for k, w in worst.items():
        if w > 1.0:
            raise AssertionError(f"{k}: fused and torch differ by {w} of the bound")
    if not all(torch.equal(a, b) for a, b in zip(gae_out["fused"], gae_out["loop"])):
        raise AssertionError("gae: fused and loop differ")

    med = {k: statistics.median(v) for k, v in ms.items()}
    loss_bytes = {tag: 4 * N * (2 * sum(nv) + len(nv) + 6 + 1) for tag, nv in heads.items()}
    gae_bytes = T * n * (4 * 4 + 1) + 4 * n
    share = lambda b, t_ms: round(b / (t_ms * 1e-3) / (args.hbm_gbs * 1e9), 4)  # noqa: E731
    line = {"tool": "tools/bench_ppo_loss.py", "T": T, "B": B, "N": N, "gae_n": n, "repeats": args.repeats,
            "settle_ms": args.settle_ms, "settle_calls": settle_calls,
            "timing": "HIP events around one graph replay (loss + backward) or one eager call (GAE), interleaved, "
                      "median of the repeats",
            "paths": {"fused_*": "ppo_loss_fused + backward (hftlob_ppo_loss: 3 launches, then two scalings by the "
                                 "upstream gradient), HIP graph",
                      "torch_*": "ppo_loss_multi + backward under autograd, HIP graph",
                      "gae_fused": "hftlob.train.loss.gae (hftlob_gae: 1 launch), eager",
                      "gae_loop": "calculate_gae (the loop over T), eager"},
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "torch_over_fused": {tag: round(med[f"torch_{tag}"] / med[f"fused_{tag}"], 3) for tag in heads},
            "gae_loop_over_fused": round(med["gae_loop"] / med["gae_fused"], 3),
            "bytes": {"loss": loss_bytes, "gae": gae_bytes},
            "hbm_gbs_assumed": args.hbm_gbs,
            "share_of_hbm_bandwidth": {**{f"fused_{tag}": share(loss_bytes[tag], med[f"fused_{tag}"]) for tag in heads},
                                       "gae_fused": share(gae_bytes, med["gae_fused"])},
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
