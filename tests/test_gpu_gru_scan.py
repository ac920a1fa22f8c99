"""The fused GRU scan on the GPU (hftlob_gru_scan_fwd / _bwd, hftlob.train.gru.GRUScan, the
learner's FUSED_GRU switch) against the float64 CPU restatement evaluated from the same float32
inputs.  Tolerance, per tensor: |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, and exactly 0 where
the whole reference tensor is 0 (a float32 torch loop on the CPU uses at most 0.025 of it)."""
import functools

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.train import gru as G
from hftlob.train import ippo as I

pytestmark = pytest.mark.gpu

# (T, B, H, every row done at t = 0 and one all-done step): one row in a tile with the h0 path only;
# exactly one full tile; a second tile with one live row; the full K loop, the column split over
# waves and three tiles; d_h0 == 0
CASES = [(1, 1, 64, False), (3, 16, 64, False), (5, 17, 128, False), (8, 33, 256, False), (4, 40, 256, True)]


def assert_close(name, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert not got.any(), f"{name}: reference is 0 everywhere, got max |x| = {float(got.abs().max())}"
        return
    excess = (got - ref).abs() - (1e-5 * ref.abs() + 1e-5 * scale)
    worst = float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * scale)).max())
    print(f"{name}: max error / bound = {worst:.4f}")
    assert float(excess.max()) <= 0.0, f"{name}: max error / bound = {worst}"


@functools.lru_cache(maxsize=None)
def case(T, B, H, all0):
    """Float32 inputs (non-zero b_hh, d_hseq non-zero at every t, done at rate 0.3) and the float64
    CPU reference of every output; computed once per shape and not modified by the tests."""
    g = torch.Generator().manual_seed(7 * T + 31 * B + H)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = torch.arange(B) % 2 == 1
    if all0:
        done[0] = True
        done[2] = True
    x = dict(gi=r(T, B, 3 * H), h0=r(B, H), done=done, w_hh=r(3 * H, H) / H ** 0.5, b_hh=0.5 * r(3 * H),
             d_hseq=r(T, B, H))
    d = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in x.items()}
    hseq, gates = G.gru_scan_reference(d["gi"], d["h0"], d["done"], d["w_hh"], d["b_hh"])
    d_gi, d_gh_n, d_h0 = G.gru_scan_backward_reference(d["d_hseq"], hseq, gates, d["h0"], d["done"], d["w_hh"])
    d_w, d_b = G.weight_grads(d_gi, d_gh_n, hseq, d["h0"], d["done"])
    ref = dict(hseq=hseq, gates=gates, d_gi=d_gi, d_gh_n=d_gh_n, d_h0=d_h0, d_w_hh=d_w, d_b_hh=d_b)
    return x, ref


def dev(x):
    return {k: v.cuda() for k, v in x.items()}


@pytest.mark.parametrize("T,B,H,all0", CASES)
def test_operators_match_float64(T, B, H, all0):
    x, ref = case(T, B, H, all0)
    c = dev(x)
    hseq, gates = G.scan_forward(c["gi"], c["h0"], c["done"], c["w_hh"], c["b_hh"], save_gates=True)
    assert_close("hseq", hseq, ref["hseq"])
    assert_close("gates", gates, ref["gates"])
    plain, none = G.scan_forward(c["gi"], c["h0"], c["done"], c["w_hh"], c["b_hh"], save_gates=False)
    assert none is None and torch.equal(plain, hseq)          # gates = NULL: the same hseq bit for bit
    # the backward operator on the float64 forward rounded to float32 (its own error alone), then on
    # the forward operator's outputs (what GRUScan feeds it)
    for label, hs, gt in (("ref fwd", ref["hseq"].float().cuda(), ref["gates"].float().cuda()), ("own fwd", hseq, gates)):
        d_gi, d_gh_n, d_h0 = G.scan_backward(c["d_hseq"], hs, gt, c["h0"], c["done"], c["w_hh"])
        assert_close(f"d_gi ({label})", d_gi, ref["d_gi"])
        assert_close(f"d_gh_n ({label})", d_gh_n, ref["d_gh_n"])
        assert_close(f"d_h0 ({label})", d_h0, ref["d_h0"])
    if all0:
        assert not ref["d_h0"].any()


@pytest.mark.parametrize("T,B,H,all0", CASES)
def test_autograd_function_matches_float64(T, B, H, all0):
    x, ref = case(T, B, H, all0)
    c = dev(x)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("gi", "h0", "w_hh", "b_hh")}
    hseq = G.gru_scan(leaves["gi"], leaves["h0"], c["done"], leaves["w_hh"], leaves["b_hh"])
    hseq.backward(c["d_hseq"])
    assert_close("hseq", hseq, ref["hseq"])
    for k, rk in (("gi", "d_gi"), ("h0", "d_h0"), ("w_hh", "d_w_hh"), ("b_hh", "d_b_hh")):
        assert_close(rk, leaves[k].grad, ref[rk])
    with torch.no_grad():                                        # no input needs a gradient: gates = NULL
        assert torch.equal(G.gru_scan(c["gi"], c["h0"], c["done"], c["w_hh"], c["b_hh"]), hseq)


def test_rows_past_B_are_not_written():
    """B = 17: the second tile has one live row.  Every output is allocated with one spare tile of
    rows behind it, filled with a sentinel that must be intact afterwards (memory the test owns)."""
    T, B, H, TILE, S = 5, 17, 128, 16, -12345.0
    x, ref = case(T, B, H, False)
    c = dev(x)
    L = _lib.lib()

    def padded(width):
        return torch.full((T * B + TILE, width), S, dtype=torch.float32, device="cuda")

    hseq, gates, d_gi, d_gh_n = padded(H), padded(4 * H), padded(3 * H), padded(H)
    d_h0 = torch.full((B + TILE, H), S, dtype=torch.float32, device="cuda")
    done = c["done"].view(torch.uint8)
    p, s = _lib.ptr, _lib.stream_ptr()
    _lib.check(L.hftlob_gru_scan_fwd(T, B, H, p(c["gi"]), p(c["h0"]), p(done), p(c["w_hh"]), p(c["b_hh"]), p(hseq),
                                     p(gates), s))
    _lib.check(L.hftlob_gru_scan_bwd(T, B, H, p(c["d_hseq"]), p(hseq), p(gates), p(c["h0"]), p(done), p(c["w_hh"]),
                                     p(d_gi), p(d_gh_n), p(d_h0), s))
    torch.cuda.synchronize()
    for name, buf, rows in (("hseq", hseq, T * B), ("gates", gates, T * B), ("d_gi", d_gi, T * B),
                            ("d_gh_n", d_gh_n, T * B), ("d_h0", d_h0, B)):
        assert bool((buf[rows:] == S).all()), f"{name}: rows past B were written"
        assert not bool((buf[:rows] == S).any()), f"{name}: a live element was not written"
        assert_close(name, buf[:rows].view(ref[name].shape), ref[name])


@functools.lru_cache(maxsize=None)
def saturated_case(H, kind):
    """case(6, 17, H, False) with saturated gates and its float64 reference, not modified by the tests.
    "hard": in rows b < 12 of every step the block b % 3 of gi (r, z or n) is +100 where (b // 3) % 2 == 0
    and -100 otherwise, so expf(-x) overflows to inf or underflows to 0 inside the sigmoid and the gate is
    exactly 0 or 1 in float32.  "scale4": gi and w_hh times 4.  Also returns the share of the bound that
    a float32 torch loop on the CPU uses, over every output."""
    T, B = 6, 17
    x = {k: v.clone() for k, v in case(T, B, H, False)[0].items()}
    if kind == "hard":
        for b in range(12):
            blk = b % 3
            x["gi"][:, b, blk * H:(blk + 1) * H] = 100.0 if (b // 3) % 2 == 0 else -100.0
    else:
        x["gi"] *= 4.0
        x["w_hh"] *= 4.0

    def restate(d):
        hseq, gates = G.gru_scan_reference(d["gi"], d["h0"], d["done"], d["w_hh"], d["b_hh"])
        d_gi, d_gh_n, d_h0 = G.gru_scan_backward_reference(d["d_hseq"], hseq, gates, d["h0"], d["done"], d["w_hh"])
        return dict(hseq=hseq, gates=gates, d_gi=d_gi, d_gh_n=d_gh_n, d_h0=d_h0)

    ref = restate({k: (v.double() if v.dtype == torch.float32 else v) for k, v in x.items()})
    f32 = restate(x)
    share = 0.0
    for k, r in ref.items():
        assert bool(torch.isfinite(f32[k]).all()), k
        bound = 1e-5 * r.abs() + 1e-5 * float(r.abs().max())
        share = max(share, float(((f32[k].double() - r).abs() / bound).max()))
    exact = int(((f32["gates"][..., :2 * H] == 0.0) | (f32["gates"][..., :2 * H] == 1.0)).sum())
    return x, ref, share, exact


def _saturated_run(H, kind):
    x, ref, share, exact = saturated_case(H, kind)
    print(f"float32 CPU restatement: {share:.4f} of the bound; {exact} r and z gates are exactly 0 or 1 in float32")
    c = dev(x)
    hseq, gates = G.scan_forward(c["gi"], c["h0"], c["done"], c["w_hh"], c["b_hh"], save_gates=True)
    d_gi, d_gh_n, d_h0 = G.scan_backward(c["d_hseq"], hseq, gates, c["h0"], c["done"], c["w_hh"])
    for name, got in (("hseq", hseq), ("gates", gates), ("d_gi", d_gi), ("d_gh_n", d_gh_n), ("d_h0", d_h0)):
        assert bool(torch.isfinite(got).all()), f"{name}: not finite"
        assert_close(name, got, ref[name])
    return share, exact


@pytest.mark.parametrize("H", [64, 128, 256])
def test_hard_saturated_gates(H):
    """sigmoidf_ is 1 / (1 + expf(-x)): at x = -100 expf overflows to inf and the gate must be 0, not NaN.
    The forward with gates, then the backward on the forward's own outputs, against float64."""
    share, exact = _saturated_run(H, "hard")
    assert share <= 0.25 and exact >= 1000                             # conditions on the fixture, from the CPU


def test_saturated_gates_at_scale_4():
    """gi and w_hh times 4 at H = 128: gate inputs of some tens, where 1 - z cancels but nothing overflows.
    (The float32 CPU loop uses 0.10 of the bound here, 0.17 at H = 64 and 0.23 at H = 256.)"""
    share, _ = _saturated_run(128, "scale4")
    assert share <= 0.25


def _net_and_batch(seed=0):
    torch.manual_seed(seed)
    net = I.ActorCriticRNN(6, 5, 64, 64).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    return net, g


def _batch(g, T=6, B=24, A=5):
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = torch.arange(B) % 2 == 1
    b = dict(h0=torch.randn(B, 64, generator=g), obs=torch.randn(T, B, 6, generator=g), done=done,
             action=torch.randint(0, A, (T, B), generator=g, dtype=torch.int32), value=torch.randn(T, B, generator=g),
             log_prob=-torch.rand(T, B, generator=g) - 0.5, adv=torch.randn(T, B, generator=g),
             tgt=torch.randn(T, B, generator=g))
    return {k: v.cuda() for k, v in b.items()}


def _loss_backward(net, b):
    logits, values = net(b["h0"], b["obs"], b["done"])
    loss = I.ppo_loss(logits, values, b["action"], b["value"], b["log_prob"], b["adv"], b["tgt"], 0.2, 0.5, 0.01)[0]
    loss.backward()
    return logits, values, loss


def test_module_forward_fused_matches_loop():
    net, g = _net_and_batch()
    b = _batch(g)
    out = {}
    for fused in (False, True):
        net.fused = fused
        net.zero_grad(set_to_none=True)
        logits, values, _ = _loss_backward(net, b)
        out[fused] = (logits.detach(), values.detach(), {n: p.grad.clone() for n, p in net.named_parameters()})
    assert_close("logits", out[True][0], out[False][0])
    assert_close("values", out[True][1], out[False][1])
    for n in out[False][2]:
        assert_close(f"grad {n}", out[True][2][n], out[False][2][n])


def test_fused_step_captures_and_replays_bit_for_bit():
    """forward + loss + backward with the fused scan inside one torch.cuda.graph (warm-up on a side
    stream, IPPOTrainer._run_step's pattern); two replays with new input contents equal the eager
    fused results bit for bit."""
    net, g = _net_and_batch(seed=3)
    net.fused = True
    static = _batch(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            _loss_backward(net, static)
    torch.cuda.current_stream().wait_stream(side)
    net.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits, values, loss = _loss_backward(net, static)
    grads = {n: p.grad for n, p in net.named_parameters()}
    for _ in range(2):
        new = _batch(g)
        for k, v in new.items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        got = (logits.clone(), values.clone(), loss.clone(), {n: v.clone() for n, v in grads.items()})
        for p in net.parameters():       # eager, on fresh gradient tensors
            p.grad = None
        e_logits, e_values, e_loss = _loss_backward(net, new)
        assert torch.equal(got[0], e_logits) and torch.equal(got[1], e_values) and torch.equal(got[2], e_loss)
        for n, p in net.named_parameters():
            assert torch.equal(got[3][n], p.grad), n
            p.grad = grads[n]            # the graph's own gradient tensors, for the next replay


def test_trainer_updates_with_fused_gru_in_the_graph():
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv
    cfg = builtin_config("2_player_fq_fqc")
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    env = MARLEnv(None, cfg, data=day, return_info=False, persistent_outputs=True)
    c = I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, TOTAL_TIMESTEPS=64 * 8 * 4,
                         FUSED_GRU=True, CUDA_GRAPHS=True)
    tr = I.IPPOTrainer(env, c)
    assert all(n.fused for n in tr.nets)
    for _ in range(3):
        m = tr.update()
        for d in m["loss"]:
            assert all(np.isfinite(float(v)) for v in d.values())
    assert [s["types"] for s in tr._steps] == [[i] for i in range(tr.n_types)]   # every type's own step
    assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in tr._steps)
    with pytest.raises(ValueError, match="FUSED_GRU needs GRU_HIDDEN_DIM"):
        I.IPPOTrainer(env, I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=32, FUSED_GRU=True))
