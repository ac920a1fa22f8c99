#!/usr/bin/env python3
"""book_process_depth_ (hftlob_book_process_depth: the message scan with the L2 depth after every
message in ONE launch) against the plain scan and against what the library offered before it.

Workload: 4096 envs of the 100/100 book, each replaying 112 consecutive messages of bench.py's
synthetic day from one of its window starts (the window's init book), n_levels = 10.  Timed with
HIP events on the launch stream:
  a  book_process_ with best-quote arrays (hftlob_book_process)
  b  book_process_depth_, depth only, every message kept
  c  the same with all_asks / all_bids
  d  112 one-message book_process_ launches, each followed by a torch get_L2_state
     (sort / unique / masked sums: the workaround without the kernel)
bench.py's practice: an untimed clock settle first (back-to-back launches for --settle-ms), then
--repeats interleaved repeats of the four, each from the restored books; the medians are reported.
(b)'s final books must equal (a)'s and (b)'s depth must equal (d)'s, and (b) must be faster than
(d), or the tool fails.  --variant labels the loaded library (HFTLOB_LIB selects it; `make
depth_both` builds the one that recomputes both sides after every message): the result is merged
into --out under that label, so one file holds both variants of the recompute rule.

    python tools/bench_book_depth.py [--envs 4096] [--msgs 112] [--repeats 9] [--variant side_rule]
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


def torch_l2_state(asks, bids, n_levels, maxint):
    """get_L2_state (JaxOrderBookArrays.py:1231-1264) restated in torch over [E, nO, 6] books."""
    import torch

    def unique_n(x, fill):  # jnp.unique(x, size=n_levels, fill_value=fill) per row
        s, _ = torch.sort(x, dim=-1)
        first = torch.ones_like(s, dtype=torch.bool)
        first[:, 1:] = s[:, 1:] != s[:, :-1]
        rank = first.to(torch.int64).cumsum(-1) - 1
        return torch.full_like(s, fill).scatter_(-1, rank, s)[:, :n_levels]

    def volume(side, prices):
        hit = side[:, None, :, 0] == prices[:, :, None]
        v = torch.where(hit, side[:, None, :, 1], 0).sum(-1, dtype=torch.int32)
        return torch.where(v < 0, 0, v)

    bp = -unique_n(-bids[..., 0], 1)
    ap = unique_n(torch.where(asks[..., 0] == -1, maxint, asks[..., 0]), -1)
    ap = torch.where(ap == -1, maxint, ap)
    bp = torch.where(bp == -1, -maxint, bp)
    return torch.stack((ap, volume(asks, ap), bp, volume(bids, bp)), -1).to(torch.int32)  # [E, L, 4]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--msgs", type=int, default=112)
    ap.add_argument("--levels", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--settle-ms", type=float, default=25.0)
    ap.add_argument("--n-msgs", type=int, default=400_000, help="synthetic day length (bench.py's default)")
    ap.add_argument("--mid", type=int, default=2_000_000)
    ap.add_argument("--variant", default="side_rule", help="label of the loaded library's recompute rule")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "book_depth_bench.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from hftlob import _lib
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.engine import book_process_, book_process_depth_
    from hftlob.env import MARLEnv

    E, M, NL = args.envs, args.msgs, args.levels
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = builtin_config(CONFIG)
    w = cfg.world_config
    day = generate_day(n_msgs=args.n_msgs, mid=args.mid, snap_every=w.n_data_msg_per_step * w.start_resolution)
    env = MARLEnv(None, cfg, data=day, device=dev, return_info=False)
    L, nO, nT = env.layout, w.nOrders, w.nTrades
    win = np.arange(E) % len(env.windows.starts)
    starts = env.windows.starts[win].astype(np.int64)
    assert (starts + M <= day.msgs.shape[0]).all()
    msgs = torch.from_numpy(np.ascontiguousarray(day.msgs[starts[:, None] + np.arange(M)[None, :]]).astype(np.int32)).to(dev)
    init = env._init_states[torch.from_numpy(win).to(dev)]
    a0 = init[:, L.off_asks:L.off_asks + 6 * nO].reshape(E, nO, 6).contiguous()
    b0 = init[:, L.off_bids:L.off_bids + 6 * nO].reshape(E, nO, 6).contiguous()
    t0 = torch.full((E, nT, 8), -1, dtype=torch.int32, device=dev)
    one = [msgs[:, k:k + 1].contiguous() for k in range(M)]
    a, b, t = a0.clone(), b0.clone(), t0.clone()
    ba = torch.empty((E, M, 2), dtype=torch.int32, device=dev)
    bb = torch.empty_like(ba)
    depth = torch.empty((E, M, NL, 4), dtype=torch.int32, device=dev)
    depth_d = torch.empty_like(depth)
    aa = torch.empty((E, M, nO, 6), dtype=torch.int32, device=dev)
    ab = torch.empty_like(aa)
    stream = torch.cuda.current_stream(dev)

    def path_a():
        book_process_(w, msgs, a, b, t, ba, bb)

    def path_b():
        book_process_depth_(w, msgs, a, b, t, NL, M, depth)

    def path_c():
        book_process_depth_(w, msgs, a, b, t, NL, M, depth, aa, ab)

    def path_d():
        for k in range(M):
            book_process_(w, one[k], a, b, t)
            depth_d[:, k] = torch_l2_state(a, b, NL, w.maxint)

    def timed(fn):
        a.copy_(a0); b.copy_(b0); t.copy_(t0)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        fn()
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), (a.clone(), b.clone(), t.clone())

    paths = {"a": path_a, "b": path_b, "c": path_c, "d": path_d}
    for fn in paths.values():  # warm-up: module load, allocator
        timed(fn)
    settle_calls, ts0 = 0, time.perf_counter()  # untimed clock settle
    while (time.perf_counter() - ts0) * 1e3 < args.settle_ms and settle_calls < 4096:
        path_b()
        settle_calls += 1
        torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):
        end = {}
        for k, fn in paths.items():
            dt, end[k] = timed(fn)
            ms[k].append(dt)
        for x, y, name in zip(end["a"], end["b"], ("asks", "bids", "trades")):
            if not torch.equal(x, y):
                raise AssertionError(f"book_process_depth_'s final {name} differ from book_process_'s")
        for x, y, name in zip(end["b"], end["c"], ("asks", "bids", "trades")):
            if not torch.equal(x, y):
                raise AssertionError(f"the final {name} differ with all_asks / all_bids")
        if not torch.equal(depth, depth_d):
            raise AssertionError("book_process_depth_'s depth differs from the per-message launches' torch get_L2_state")
        if not (torch.equal(aa[:, -1], end["c"][0]) and torch.equal(ab[:, -1], end["c"][1])):
            raise AssertionError("all_asks[-1] / all_bids[-1] differ from the final sides")
    med = {k: statistics.median(v) for k, v in ms.items()}
    if not med["b"] < med["d"]:
        raise AssertionError(f"the depth kernel ({med['b']:.3f} ms) is not faster than the workaround ({med['d']:.3f} ms)")
    res = {"ms": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "msgs_per_s": {k: round(E * M / (v * 1e-3), 1) for k, v in med.items()},
           "b_over_a": round(med["b"] / med["a"], 3), "c_over_a": round(med["c"] / med["a"], 3),
           "d_over_b": round(med["d"] / med["b"], 3), "outputs_equal": True, "settle_calls": settle_calls,
           "library": os.path.relpath(_lib.LIB_PATH, ROOT)}
    line = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            line = json.loads(f.read())
    line.update({"tool": "tools/bench_book_depth.py", "config": f"{CONFIG} world config ({nO}/{nT} book)", "envs": E,
                 "msgs_per_call": M, "n_levels": NL, "repeats": args.repeats, "settle_ms": args.settle_ms,
                 "timing": "HIP events on the launch stream, median of the repeats",
                 "paths": {"a": "book_process_ with best-quote arrays (hftlob_book_process)",
                           "b": "book_process_depth_, depth only, all messages kept (hftlob_book_process_depth)",
                           "c": "book_process_depth_ with depth, all_asks and all_bids",
                           "d": f"{M} one-message book_process_ launches, each followed by a torch get_L2_state"},
                 "device": torch.cuda.get_device_properties(dev).gcnArchName,
                 "data": f"synthetic LOBSTER day ({args.n_msgs} msgs, mid {args.mid})"})
    line.setdefault("variants", {})[args.variant] = res
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
