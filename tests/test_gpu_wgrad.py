"""The narrow layers' weight gradient on the GPU (hftlob_xty, hftlob.train.wgrad.xty / narrow_linear, the
learner's FUSED_WGRAD switch) against the float64 CPU restatement (xty_reference) evaluated from the same
float32 inputs.  Tolerance, per tensor: |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, and exactly 0 where the
whole reference tensor is 0.  Every fixture is checked on the CPU to leave room: a float32 ``A.t() @ B``
uses at most 0.25 of that bound."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hftlob import _lib
from hftlob.train import ippo as I
from hftlob.train import wgrad as W

pytestmark = pytest.mark.gpu

R, G = W.STRIPE_ROWS, W.MAX_STRIPES


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


def share_of_bound(got, ref):
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * ref.abs().max())).max())


# row-tile and unroll edges inside one stripe; the second stripe with one row; the cap, where the stripes grow
ROWS = [1, 3, 4, 5, 15, 16, 17, R - 1, R, R + 1, G * R, G * R + 1]
SHAPES = ([(R + 1, P, Q) for P in (1, 2, 10, 13, 16, 17, 64) for Q in (64, 128, 256)]
          + [(N, P, Q) for N in ROWS if N != R + 1 for P, Q in ((13, 256), (2, 64))])


@functools.lru_cache(maxsize=None)
def case(N, P, Q):
    """Standard-normal A [N, P] and B [N, Q] (float32, CPU) and their float64 reference; never modified.
    Past 4099 rows the values are rounded to multiples of 1/8: a float32 sum of 65 536 unrounded products
    uses 0.2 to 0.6 of the bound by itself, depending on the order the host's BLAS adds them in, while sums of
    multiples of 1/64 of this size are exact in float32 in any order, so the long cases check that every row
    of every stripe is counted once and leave the rounding to the short ones."""
    g = torch.Generator().manual_seed(1000 * P + Q + N % 997)
    A, B = torch.randn(N, P, generator=g), torch.randn(N, Q, generator=g)
    if N > 4099:
        A, B = (A * 8).round() / 8, (B * 8).round() / 8
    ref = W.xty_reference(A.double(), B.double())
    # the condition on a fixture: float32 on the CPU leaves three quarters of the bound to the kernel's order
    used = share_of_bound(A.t() @ B, ref[0])
    assert used <= 0.25, f"fixture ({N}, {P}, {Q}): a float32 A.t() @ B uses {used} of the bound"
    return A, B, ref


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_against_float64_and_same_bits(N, P, Q):
    A, B, ref = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    c, sa, sb = W.xty(a, b, want_sum_a=True, want_sum_b=True)
    assert c.shape == (P, Q) and sa.shape == (P,) and sb.shape == (Q,)
    assert_close("C", c, ref[0])
    assert_close("sum_a", sa, ref[1])
    assert_close("sum_b", sb, ref[2])
    # the same bits a second time, and C's bits whatever sums are asked for
    c2, sa2, sb2 = W.xty(a, b, want_sum_a=True, want_sum_b=True)
    assert torch.equal(c, c2) and torch.equal(sa, sa2) and torch.equal(sb, sb2)
    c3, n1, n2 = W.xty(a, b)
    assert n1 is None and n2 is None and torch.equal(c, c3)
    c4, sa4, n2 = W.xty(a, b, want_sum_a=True)
    assert n2 is None and torch.equal(c, c4) and torch.equal(sa, sa4)
    c5, n1, sb5 = W.xty(a, b, want_sum_b=True)
    assert n1 is None and torch.equal(c, c5) and torch.equal(sb, sb5)


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_zero_columns_give_exact_zeros(N, P, Q):
    A, B, _ = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    z = P // 2
    a[:, z] = 0.0
    c, sa, _ = W.xty(a, b, want_sum_a=True, want_sum_b=True)
    assert not c[z].any() and float(sa[z]) == 0.0
    if P > 1:
        assert c[[p for p in range(P) if p != z]].any()
    c, sa, sb = W.xty(torch.zeros_like(a), b, want_sum_a=True, want_sum_b=True)
    assert not c.any() and not sa.any()
    assert_close("sum_b beside a zero A", sb, B.double().sum(0))


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_rows_past_n_are_not_read(N, P, Q):
    """A and B inside larger buffers whose rows past N are NaN: finite, and the bits of exactly-sized copies."""
    A, B, _ = case(N, P, Q)
    spare = 9
    abuf = torch.full((N + spare, P), float("nan"), device="cuda")
    bbuf = torch.full((N + spare, Q), float("nan"), device="cuda")
    abuf[:N].copy_(A)
    bbuf[:N].copy_(B)
    av, bv = abuf[:N], bbuf[:N]
    assert av.is_contiguous() and av.data_ptr() == abuf.data_ptr() and bv.data_ptr() == bbuf.data_ptr()
    got = W.xty(av, bv, want_sum_a=True, want_sum_b=True)
    exact = W.xty(A.cuda(), B.cuda(), want_sum_a=True, want_sum_b=True)
    for x, y in zip(got, exact):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_outputs_are_written_and_not_overrun(N, P, Q):
    """C, the sums and the workspace with a sentinel tail behind their documented sizes: the tails are
    intact, every live element of C and the sums is written, and the bits are those of ``xty``."""
    A, B, _ = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    L = _lib.lib()
    n_ws = L.hftlob_xty_workspace(N, P, Q)
    assert n_ws == W.workspace_floats(N, P, Q) > 0
    TAIL, SENT = 256, -7777.0

    def guarded(n):
        t = torch.full((n + TAIL,), SENT, device="cuda")
        t[:n] = float("nan")
        return t

    c, sa, sb, ws = guarded(P * Q), guarded(P), guarded(Q), guarded(n_ws)
    _lib.check(L.hftlob_xty(N, P, Q, a.data_ptr(), b.data_ptr(), c.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                            ws.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    want = W.xty(a, b, want_sum_a=True, want_sum_b=True)
    for name, buf, n, w in (("C", c, P * Q, want[0]), ("sum_a", sa, P, want[1]), ("sum_b", sb, Q, want[2])):
        assert bool((buf[n:] == SENT).all()), f"{name}: the tail was written"
        assert bool(torch.isfinite(buf[:n]).all()), f"{name}: a live element was not written"
        assert torch.equal(buf[:n], w.reshape(-1)), name
    assert bool((ws[n_ws:] == SENT).all()), "workspace: the tail was written"
    assert bool(torch.isfinite(ws[:n_ws]).all()), "workspace: a partial was not written"


def test_empty_batch_gives_zeros():
    c, sa, sb = W.xty(torch.empty(0, 13, device="cuda"), torch.empty(0, 256, device="cuda"), True, True)
    torch.cuda.synchronize()
    assert c.shape == (13, 256) and not c.any() and not sa.any() and not sb.any()


def test_wrapper_refuses_bad_tensors():
    a, b = torch.zeros(4, 13, device="cuda"), torch.zeros(4, 256, device="cuda")
    with pytest.raises(ValueError, match="needs A"):
        W.xty(a, b[:3])
    with pytest.raises(RuntimeError, match="device"):
        W.xty(a.cpu(), b.cpu())
    with pytest.raises(_lib.HftlobError, match="Q must be"):
        W.xty(a, torch.zeros(4, 96, device="cuda"))
    with pytest.raises(_lib.HftlobError, match="P must be"):
        W.xty(torch.zeros(4, 65, device="cuda"), b)


# ------------------------------------------------------------------ narrow_linear
def _linear_case(in_f, out_f, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5, 17, in_f, generator=g)
    w = torch.randn(out_f, in_f, generator=g) / in_f ** 0.5
    b = torch.randn(out_f, generator=g)
    return x, w, b, g


def _losses(out_f):
    """Ways from y [5, 17, out_f] to a scalar, by what they hand the layer as d_y."""
    g = torch.Generator().manual_seed(out_f)
    wt = torch.randn(5, 17, out_f, generator=g)
    ways = {"dense": lambda y, k: (y * k(wt)).sum(),
            "transposed": lambda y, k: (y.transpose(0, 1) * k(wt.transpose(0, 1))).sum()}
    if out_f == 1:
        ways["squeeze"] = lambda y, k: (y.squeeze(-1) * k(wt[..., 0])).sum()
    else:
        cut = [out_f // 3, out_f - out_f // 3]
        ways["split"] = lambda y, k: sum((part * k(wp)).sum() for part, wp in zip(y.split(cut, -1), wt.split(cut, -1)))
    return ways


@pytest.mark.parametrize("in_f,out_f", [(64, 13), (256, 1), (128, 7), (12, 64), (2, 256), (64, 64)])
def test_narrow_linear_both_orientations(in_f, out_f):
    x0, w0, b0, _ = _linear_case(in_f, out_f, in_f + out_f)
    for name, loss in _losses(out_f).items():
        for with_bias in (True, False):
            for x_grad in (True, False):
                leaf = lambda t, dt, dev, rg=True: t.to(dev, dt).clone().requires_grad_(rg)   # noqa: E731
                # float64 autograd on the CPU, torch's float32 layer on the GPU, and narrow_linear
                x64, w64 = leaf(x0, torch.float64, "cpu", x_grad), leaf(w0, torch.float64, "cpu")
                b64 = leaf(b0, torch.float64, "cpu") if with_bias else None
                loss(F.linear(x64, w64, b64), lambda t: t.double()).backward()
                xt, wt = leaf(x0, torch.float32, "cuda", x_grad), leaf(w0, torch.float32, "cuda")
                bt = leaf(b0, torch.float32, "cuda") if with_bias else None
                yt = F.linear(xt, wt, bt)
                loss(yt, lambda t: t.cuda()).backward()
                xn, wn = leaf(x0, torch.float32, "cuda", x_grad), leaf(w0, torch.float32, "cuda")
                bn = leaf(b0, torch.float32, "cuda") if with_bias else None
                yn = W.narrow_linear(xn, wn, bn)
                loss(yn, lambda t: t.cuda()).backward()
                tag = f"{name} bias={with_bias} x_grad={x_grad}"
                assert torch.equal(yn, yt), tag
                if x_grad:
                    assert torch.equal(xn.grad, xt.grad), tag
                else:
                    assert xn.grad is None
                assert wn.grad.shape == wn.shape and wn.grad.is_contiguous()
                assert_close(f"d_w {tag}", wn.grad, w64.grad)
                if with_bias:
                    assert_close(f"d_b {tag}", bn.grad, b64.grad)


# ------------------------------------------------------------------ the module
def _batch(g, D, heads, T=6, B=24, H=64):
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = torch.arange(B) % 2 == 1
    action = torch.stack([torch.randint(0, n, (T, B), generator=g, dtype=torch.int32) for n in heads], -1)
    b = dict(h0=torch.randn(B, H, generator=g), obs=torch.randn(T, B, D, generator=g), done=done, action=action,
             value=torch.randn(T, B, generator=g), log_prob=-torch.rand(T, B, generator=g) - 0.5,
             adv=torch.randn(T, B, generator=g), tgt=torch.randn(T, B, generator=g))
    return {k: v.cuda() for k, v in b.items()}


def _loss_backward(net, b):
    logits, values = net(b["h0"], b["obs"], b["done"])
    loss = I.ppo_loss_multi(logits, values, b["action"], b["value"], b["log_prob"], b["adv"], b["tgt"], 0.2, 0.5, 0.01,
                            net.heads)[0]
    loss.backward()
    return logits, values, loss


@pytest.mark.parametrize("fused", [False, True], ids=["loop", "fused_scan"])
@pytest.mark.parametrize("D,A", [(12, 13), (12, [3, 4]), (2, 10)], ids=["d12_a13", "multidiscrete_3_4", "d2_a10"])
def test_module_with_the_switch_matches_the_module_without(D, A, fused):
    torch.manual_seed(5)
    net = I.ActorCriticRNN(D, A, 64, 64).cuda()
    net.fused = fused
    b = _batch(torch.Generator().manual_seed(6), D, net.heads)
    out = {}
    for on in (False, True):
        net.fused_wgrad = on
        net.zero_grad(set_to_none=True)
        logits, values, loss = _loss_backward(net, b)
        out[on] = (logits.detach(), values.detach(), loss.detach(),
                   {n: p.grad.clone() for n, p in net.named_parameters()})
    assert all(torch.equal(x, y) for x, y in zip(out[True][:3], out[False][:3]))
    for n, ref in out[False][3].items():
        assert_close(f"grad {n}", out[True][3][n], ref)
        if not n.startswith(("embed", "actor2", "critic2")):     # nothing upstream of them changed
            assert torch.equal(out[True][3][n], ref), n


@pytest.mark.parametrize("fused", [False, True], ids=["loop", "fused_scan"])
def test_step_with_the_switch_captures_and_replays_bit_for_bit(fused):
    """forward + loss + backward with fused_wgrad inside one torch.cuda.graph (warm-up on a side stream,
    IPPOTrainer._run_step's pattern); two replays with new input contents equal the eager results bit
    for bit."""
    torch.manual_seed(3)
    net = I.ActorCriticRNN(12, 13, 64, 64).cuda()
    net.fused, net.fused_wgrad = fused, True
    g = torch.Generator().manual_seed(4)
    static = _batch(g, 12, net.heads)
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
        new = _batch(g, 12, net.heads)
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


# ------------------------------------------------------------------ the trainer
@functools.lru_cache(maxsize=None)
def _env():
    from hftlob.config_io import builtin_config
    from hftlob.data.synthetic import generate_day
    from hftlob.env import MARLEnv
    cfg = builtin_config("2_player_fq_fqc")
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=False, persistent_outputs=True)


def _config(**kw):
    return I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, TOTAL_TIMESTEPS=64 * 8 * 4,
                            CUDA_GRAPHS=True, FUSED_GRU=True, FUSED_POLICY=True, FUSED_LOSS=True, FUSED_OPT=True,
                            FUSED_WGRAD=True, **kw)


def test_trainer_updates_with_every_switch_per_type_and_grouped():
    runs = []
    for grouped in (False, True):
        tr = I.IPPOTrainer(_env(), _config(GROUPED_SCAN=grouped))
        assert tr.fused_wgrad and all(n.fused_wgrad and n.fused for n in tr.nets)
        for _ in range(3):
            m = tr.update()
            assert all(np.isfinite(float(v)) for d in m["loss"] for v in d.values())
        if grouped:
            assert [s["types"] for s in tr._steps] == [list(range(tr.n_types))]   # the one joint step
            assert isinstance(tr._steps[0]["graph"], torch.cuda.CUDAGraph)
        else:
            assert [s["types"] for s in tr._steps] == [[i] for i in range(tr.n_types)]   # every type's own step
            assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in tr._steps)
        runs.append(tr)
    torch.cuda.synchronize()
    a, b = runs   # the operator is the same per net either way: the same training, bit for bit
    assert a.opt_count == b.opt_count
    for i in range(a.n_types):
        for (name, p), q in zip(a.nets[i].named_parameters(), b.nets[i].parameters()):
            assert torch.equal(p, q), f"type {i}: {name}"
            sa, sb = a.opts[i].state[p], b.opts[i].state[q]
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sa[key], sb[key]), f"type {i}: {name} {key}"


def test_trainer_refuses_sizes_the_operator_does_not_take():
    with pytest.raises(ValueError, match="FUSED_WGRAD needs GRU_HIDDEN_DIM and FC_DIM_SIZE in"):
        I.IPPOTrainer(_env(), I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=32, FUSED_WGRAD=True))
