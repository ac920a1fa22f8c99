"""The wide layers' weight gradient on the GPU (hftlob_xty_wide, hftlob.train.wgrad.xty_wide / wide_linear,
train.gru.weight_grads_fused, the learner's FUSED_WGRAD_WIDE switch) against the float64 CPU restatement
(xty_wide_reference) evaluated from the same float32 inputs.  Tolerance, per tensor, that of
tests/test_gpu_wgrad.py: |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, and exactly 0 where the whole reference
tensor is 0.  Every fixture is checked on the CPU to leave room: a float32 ``A.t() @ B`` uses at most 0.25 of
that bound."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hftlob import _lib
from hftlob.train import gru as GR
from hftlob.train import ippo as I
from hftlob.train import wgrad as W

pytestmark = pytest.mark.gpu

R, KC = W.WIDE_STRIPE_ROWS, W.WIDE_CHUNK


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


def _edges(P, Q):
    """N at the edges of the row walk: single rows, the LDS chunk, one stripe, and the cap, where the stripes grow."""
    M = W.wide_max_stripes(P, Q)
    return [1, 2, 3, KC - 1, KC, KC + 1, R - 1, R, M * R, M * R + 1]


SHAPES = ([(R + 1, P, Q) for P in (64, 128, 192, 256, 384, 768) for Q in (64, 128, 256)]
          + [(N, P, Q) for P, Q in ((768, 256), (64, 64)) for N in _edges(P, Q)])
SPLIT = [s for s in SHAPES if s[1] >= 128]    # the shapes whose A can come as two blocks


@functools.lru_cache(maxsize=None)
def case(N, P, Q):
    """Standard-normal A [N, P] and B [N, Q] (float32, CPU) and their float64 reference; never modified.
    Past 4099 rows the values are multiples of 1/8 (tests/test_gpu_wgrad.py's rule and reason): the long cases
    check that every row of every stripe is counted once and leave the rounding to the short ones."""
    g = torch.Generator().manual_seed(1000 * P + Q + N % 997)
    A, B = torch.randn(N, P, generator=g), torch.randn(N, Q, generator=g)
    if N > 4099:
        A, B = (A * 8).round() / 8, (B * 8).round() / 8
    ref = W.xty_wide_reference([A.double()], B.double())
    used = share_of_bound(A.t() @ B, ref[0])
    assert used <= 0.25, f"fixture ({N}, {P}, {Q}): a float32 A.t() @ B uses {used} of the bound"
    return A, B, ref


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_against_float64_and_same_bits(N, P, Q):
    A, B, ref = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    c, sa = W.xty_wide([a], b, want_sum_a=True)
    assert c.shape == (P, Q) and sa.shape == (P,)
    assert_close("C", c, ref[0])
    assert_close("sum_a", sa, ref[1])
    # the same bits a second time, and C's bits whether or not the sums are asked for
    c2, sa2 = W.xty_wide([a], b, want_sum_a=True)
    assert torch.equal(c, c2) and torch.equal(sa, sa2)
    c3, none = W.xty_wide([a], b)
    assert none is None and torch.equal(c, c3)


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_zero_columns_give_exact_zeros(N, P, Q):
    A, B, _ = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    z = P // 2 + 1
    a[:, z] = 0.0
    c, sa = W.xty_wide([a], b, want_sum_a=True)
    assert not c[z].any() and float(sa[z]) == 0.0
    assert c[[p for p in range(P) if p != z]].any()
    c, sa = W.xty_wide([torch.zeros_like(a)], b, want_sum_a=True)
    assert not c.any() and not sa.any()


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_rows_past_n_are_not_read(N, P, Q):
    """A and B inside larger buffers whose rows past N are NaN, and with a shift the rows N - shift .. of B
    NaN as well: finite, and the bits of exactly-sized copies."""
    A, B, _ = case(N, P, Q)
    spare = 9
    abuf = torch.full((N + spare, P), float("nan"), device="cuda")
    bbuf = torch.full((N + spare, Q), float("nan"), device="cuda")
    abuf[:N].copy_(A)
    bbuf[:N].copy_(B)
    av, bv = abuf[:N], bbuf[:N]
    assert av.is_contiguous() and av.data_ptr() == abuf.data_ptr() and bv.data_ptr() == bbuf.data_ptr()
    got = W.xty_wide([av], bv, want_sum_a=True)
    exact = W.xty_wide([A.cuda()], B.cuda(), want_sum_a=True)
    for x, y in zip(got, exact):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    shift = min(N, 5)
    head = B[:shift].flip(0).contiguous().cuda()
    bbuf[N - shift:] = float("nan")
    got = W.xty_wide([av], bbuf[:N], head, shift, want_sum_a=True)
    exact = W.xty_wide([A.cuda()], B[:N - shift].contiguous().cuda(), head, shift, want_sum_a=True)
    for x, y in zip(got, exact):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("N,P,Q", SHAPES)
def test_outputs_are_written_and_not_overrun(N, P, Q):
    """C, sum_a and the workspace with a sentinel tail behind their documented sizes: the tails are intact,
    every live element is written, and the bits are those of ``xty_wide``."""
    A, B, _ = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    L = _lib.lib()
    n_ws = L.hftlob_xty_wide_workspace(N, P, Q)
    assert n_ws == W.wide_workspace_floats(N, P, Q) > 0
    TAIL, SENT = 256, -7777.0

    def guarded(n):
        t = torch.full((n + TAIL,), SENT, device="cuda")
        t[:n] = float("nan")
        return t

    c, sa, ws = guarded(P * Q), guarded(P), guarded(n_ws)
    _lib.check(L.hftlob_xty_wide(N, Q, a.data_ptr(), P, P, None, 0, 0, b.data_ptr(), None, 0, None, c.data_ptr(),
                                 sa.data_ptr(), ws.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    want = W.xty_wide([a], b, want_sum_a=True)
    for name, buf, n, w in (("C", c, P * Q, want[0]), ("sum_a", sa, P, want[1])):
        assert bool((buf[n:] == SENT).all()), f"{name}: the tail was written"
        assert bool(torch.isfinite(buf[:n]).all()), f"{name}: a live element was not written"
        assert torch.equal(buf[:n], w.reshape(-1)), name
    assert bool((ws[n_ws:] == SENT).all()), "workspace: the tail was written"
    assert bool(torch.isfinite(ws[:n_ws]).all()), "workspace: a partial was not written"


@pytest.mark.parametrize("N,P,Q", SPLIT)
def test_two_strided_blocks_equal_the_concatenated_a(N, P, Q):
    A, B, _ = case(N, P, Q)
    a, b = A.cuda(), B.cuda()
    want = W.xty_wide([a], b, want_sum_a=True)
    for cols0 in {64, P - 64, (P // 128) * 64}:
        # block 0 the first columns of a wider tensor (a row stride past its columns), block 1 its own tensor
        wide = torch.full((N, cols0 + 64), float("nan"), device="cuda")
        wide[:, :cols0] = a[:, :cols0]
        rest = a[:, cols0:].contiguous()
        got = W.xty_wide([wide[:, :cols0], rest], b, want_sum_a=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), cols0
        # and both blocks views of the one tensor
        got = W.xty_wide([a[:, :cols0], a[:, cols0:]], b, want_sum_a=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), cols0


@pytest.mark.parametrize("N,P,Q", [(2 * R + 5, 768, 256), (2 * R + 5, 64, 64), (R + 1, 192, 128), (3, 128, 64)])
def test_shifted_and_masked_b_equals_the_materialised_rows(N, P, Q):
    A, B, _ = case(N, P, Q)
    g = torch.Generator().manual_seed(N)
    a, b = A.cuda(), B.cuda()
    masks = [None, torch.rand(N, generator=g) < 0.3]
    if N > 2 * R:
        whole = torch.zeros(N, dtype=torch.bool)
        whole[R:2 * R] = True                                     # all of stripe 1
        masks.append(whole)
    for shift in sorted({0, 1, min(24, N), N}):
        head = torch.randn(shift, Q, generator=g)
        for mask in masks:
            for h in (head, None):
                ref = W.xty_wide_reference([A.double()], B.double(), None if h is None else h.double(), shift, mask)
                rows = torch.cat([head if h is not None else torch.zeros_like(head), B[:N - shift]])
                if mask is not None:
                    rows = torch.where(mask[:, None], torch.zeros_like(rows), rows)
                want = W.xty_wide([a], rows.cuda(), want_sum_a=True)
                bnan = b.clone()
                bnan[N - shift:] = float("nan")
                if mask is not None:                              # a masked row's value is not used
                    bnan[:N - shift][mask[shift:].cuda()] = float("nan")
                got = W.xty_wide([a], bnan, None if h is None else h.cuda(), shift,
                                 None if mask is None else mask.cuda(), want_sum_a=True)
                tag = f"shift {shift}, mask {None if mask is None else int(mask.sum())}, head {h is not None}"
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), tag
                assert_close(f"C {tag}", got[0], ref[0])


def test_empty_batch_gives_zeros():
    c, sa = W.xty_wide([torch.empty(0, 192, device="cuda")], torch.empty(0, 256, device="cuda"), want_sum_a=True)
    torch.cuda.synchronize()
    assert c.shape == (192, 256) and not c.any() and sa.shape == (192,) and not sa.any()


def test_wrapper_refuses_bad_tensors():
    a, b = torch.zeros(4, 128, device="cuda"), torch.zeros(4, 256, device="cuda")
    with pytest.raises(ValueError, match="needs A's blocks"):
        W.xty_wide([a], b[:3])
    with pytest.raises(RuntimeError, match="device"):
        W.xty_wide([a.cpu()], b.cpu())
    with pytest.raises(_lib.HftlobError, match="Q must be"):
        W.xty_wide([a], torch.zeros(4, 96, device="cuda"))
    with pytest.raises(_lib.HftlobError, match="multiple of 64"):
        W.xty_wide([torch.zeros(4, 96, device="cuda")], b)
    with pytest.raises(_lib.HftlobError, match="P must be"):
        W.xty_wide([torch.zeros(4, 512, device="cuda"), torch.zeros(4, 320, device="cuda")], b)
    with pytest.raises(_lib.HftlobError, match="16-byte aligned"):
        W.xty_wide([torch.zeros(4, 132, device="cuda")[:, 2:130]], b)


# ------------------------------------------------------------------ wide_linear
def _linear_case(in_f, out_f, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5, 17, in_f, generator=g)
    w = torch.randn(out_f, in_f, generator=g) / in_f ** 0.5
    b = torch.randn(out_f, generator=g)
    return x, w, b


def _losses(out_f):
    """Ways from y [5, 17, out_f] to a scalar, by what they hand the layer as d_y."""
    g = torch.Generator().manual_seed(out_f)
    wt = torch.randn(5, 17, out_f, generator=g)
    return {"dense": lambda y, k: (y * k(wt)).sum(),
            "transposed": lambda y, k: (y.transpose(0, 1) * k(wt.transpose(0, 1))).sum()}


@pytest.mark.parametrize("in_f,out_f", [(64, 192), (256, 256), (128, 64)])
def test_wide_linear(in_f, out_f):
    x0, w0, b0 = _linear_case(in_f, out_f, in_f + out_f)
    for name, loss in _losses(out_f).items():
        for with_bias in (True, False):
            for x_grad in (True, False):
                leaf = lambda t, dt, dev, rg=True: t.to(dev, dt).clone().requires_grad_(rg)   # noqa: E731
                # float64 autograd on the CPU, torch's float32 layer on the GPU, and wide_linear
                x64, w64 = leaf(x0, torch.float64, "cpu", x_grad), leaf(w0, torch.float64, "cpu")
                b64 = leaf(b0, torch.float64, "cpu") if with_bias else None
                loss(F.linear(x64, w64, b64), lambda t: t.double()).backward()
                xt, wt = leaf(x0, torch.float32, "cuda", x_grad), leaf(w0, torch.float32, "cuda")
                bt = leaf(b0, torch.float32, "cuda") if with_bias else None
                yt = F.linear(xt, wt, bt)
                loss(yt, lambda t: t.cuda()).backward()
                xn, wn = leaf(x0, torch.float32, "cuda", x_grad), leaf(w0, torch.float32, "cuda")
                bn = leaf(b0, torch.float32, "cuda") if with_bias else None
                yn = W.wide_linear(xn, wn, bn)
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


# ------------------------------------------------------------------ weight_grads_fused
@pytest.mark.parametrize("T,B,H", [(6, 24, 64), (6, 17, 64)])
def test_weight_grads_fused(T, B, H):
    g = torch.Generator().manual_seed(T * B)
    d_gi, d_gh_n = torch.randn(T, B, 3 * H, generator=g), torch.randn(T, B, H, generator=g)
    hseq, h0 = torch.randn(T, B, H, generator=g), torch.randn(B, H, generator=g)
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = torch.arange(B) % 2 == 1
    ref = GR.weight_grads(d_gi.double(), d_gh_n.double(), hseq.double(), h0.double(), done)
    dev = [t.cuda() for t in (d_gi, d_gh_n, hseq, h0, done)]
    d_w, d_b = GR.weight_grads_fused(*dev)
    assert d_w.shape == (3 * H, H) and d_b.shape == (3 * H,)
    assert_close("d_w_hh", d_w, ref[0])
    assert_close("d_b_hh", d_b, ref[1])
    again = GR.weight_grads_fused(*dev)
    assert torch.equal(again[0], d_w) and torch.equal(again[1], d_b)


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
def test_module_with_the_switch_matches_the_module_without(fused):
    torch.manual_seed(5)
    net = I.ActorCriticRNN(12, 13, 64, 64).cuda()
    net.fused = fused
    b = _batch(torch.Generator().manual_seed(6), 12, net.heads)
    out = {}
    for on in (False, True):
        net.fused_wgrad_wide = on
        net.zero_grad(set_to_none=True)
        logits, values, loss = _loss_backward(net, b)
        out[on] = (logits.detach(), values.detach(), loss.detach(),
                   {n: p.grad.clone() for n, p in net.named_parameters()})
    assert all(torch.equal(x, y) for x, y in zip(out[True][:3], out[False][:3]))
    for n, ref in out[False][3].items():
        assert_close(f"grad {n}", out[True][3][n], ref)
        if n.startswith(("embed", "actor2", "critic2")):         # nothing upstream of them changed
            assert torch.equal(out[True][3][n], ref), n
        if not fused and n in ("gru.weight_hh", "gru.bias_hh"):  # the loop scan's stay autograd's
            assert torch.equal(out[True][3][n], ref), n


@pytest.mark.parametrize("fused", [False, True], ids=["loop", "fused_scan"])
def test_step_with_the_switch_captures_and_replays_bit_for_bit(fused):
    """forward + loss + backward with fused_wgrad_wide inside one torch.cuda.graph (warm-up on a side stream,
    IPPOTrainer._run_step's pattern); two replays with new input contents equal the eager results bit for
    bit."""
    torch.manual_seed(3)
    net = I.ActorCriticRNN(12, 13, 64, 64).cuda()
    net.fused, net.fused_wgrad_wide = fused, True
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
                            FUSED_WGRAD=True, FUSED_WGRAD_WIDE=True, **kw)


def test_trainer_updates_with_every_switch_per_type_and_grouped():
    runs = []
    for grouped in (False, True):
        tr = I.IPPOTrainer(_env(), _config(GROUPED_SCAN=grouped))
        assert tr.fused_wgrad_wide and all(n.fused_wgrad_wide and n.fused_wgrad and n.fused for n in tr.nets)
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
    with pytest.raises(ValueError, match="FUSED_WGRAD_WIDE needs GRU_HIDDEN_DIM and FC_DIM_SIZE in"):
        I.IPPOTrainer(_env(), I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=32, FUSED_WGRAD_WIDE=True))
