"""The wide layers' weight gradient without a GPU: the torch restatement (hftlob.train.wgrad.xty_wide_reference)
against a float64 einsum, with strided blocks, the shifted and masked B and NaN where nothing may be read;
train.gru.weight_grads_fused's operands against weight_grads; the header's constants and declarations; the
stripe rule and the workspace size against the built library; the argument checks of hftlob_xty_wide (they
run before any device work), in the documented order; and the trainer's FUSED_WGRAD_WIDE switch on a CPU
device."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from hftlob import _lib
from hftlob.train import gru as GR
from hftlob.train import ippo as I
from hftlob.train import wgrad as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")
OK, EINVAL, ENULL, ESHAPE = 0, -1, -2, -3
R = W.WIDE_STRIPE_ROWS


@pytest.mark.parametrize("N,P,Q", [(1, 64, 64), (7, 192, 128), (33, 256, 256), (130, 768, 64)])
def test_reference_is_the_transposed_product_and_the_column_sums(N, P, Q):
    g = torch.Generator().manual_seed(N + P)
    A = torch.randn(N, P, generator=g, dtype=torch.float64)
    B = torch.randn(N, Q, generator=g, dtype=torch.float64)
    c, sa = W.xty_wide_reference([A], B)
    assert c.dtype == torch.float64 and c.shape == (P, Q) and sa.shape == (P,)
    torch.testing.assert_close(c, torch.einsum("np,nq->pq", A, B), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(sa, torch.einsum("np->p", A), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("N,shift", [(40, 0), (40, 1), (40, 8), (40, 40)])
def test_reference_with_strided_blocks_shift_head_and_mask(N, shift):
    g = torch.Generator().manual_seed(N + shift)
    wide = torch.randn(N, 192, generator=g, dtype=torch.float64)
    other = torch.randn(N, 64, generator=g, dtype=torch.float64)
    blocks = [wide[:, :128], other]                               # the first block has a row stride of 192
    assert blocks[0].stride(0) == 192
    Q = 64
    B = torch.randn(N, Q, generator=g, dtype=torch.float64)
    B[N - shift:] = float("nan")                                  # rows N - shift .. are never read
    head = torch.randn(shift, Q, generator=g, dtype=torch.float64)
    mask = torch.rand(N, generator=g) < 0.3
    # the rows of B' written out one by one
    rows = torch.stack([torch.zeros(Q, dtype=torch.float64) if mask[n] else (head[n] if n < shift else B[n - shift])
                        for n in range(N)])
    A = torch.cat(blocks, 1)
    want = torch.einsum("np,nq->pq", A, rows)
    c, sa = W.xty_wide_reference(blocks, B, head, shift, mask)
    assert bool(torch.isfinite(c).all())
    torch.testing.assert_close(c, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(sa, A.sum(0), rtol=1e-12, atol=1e-12)
    # a masked row's value is not used either
    B2 = B.clone()
    B2[:N - shift][mask[shift:]] = float("nan")
    assert torch.equal(W.xty_wide_reference(blocks, B2, head, shift, mask)[0], c)
    # no mask, and no head (zeros)
    c, _ = W.xty_wide_reference(blocks, B, head, shift)
    rows = torch.cat([head, B[:N - shift]])
    torch.testing.assert_close(c, torch.einsum("np,nq->pq", A, rows), rtol=1e-12, atol=1e-12)
    c, _ = W.xty_wide_reference(blocks, B, None, shift)
    rows = torch.cat([torch.zeros_like(head), B[:N - shift]])
    torch.testing.assert_close(c, torch.einsum("np,nq->pq", A, rows), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T,B,H", [(6, 24, 64), (5, 17, 64), (1, 3, 128)])
def test_fused_operands_restate_weight_grads(T, B, H):
    g = torch.Generator().manual_seed(T + B)
    d_gi = torch.randn(T, B, 3 * H, generator=g, dtype=torch.float64)
    d_gh_n = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    hseq = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    h0 = torch.randn(B, H, generator=g, dtype=torch.float64)
    done = torch.rand(T, B, generator=g) < 0.3
    done[0, ::2] = True
    blocks, rows, head, shift, zero_row = GR.fused_wgrad_operands(d_gi, d_gh_n, hseq, h0, done)
    assert shift == B and blocks[0].shape == (T * B, 2 * H) and blocks[0].stride(0) == 3 * H
    assert blocks[0].data_ptr() == d_gi.data_ptr() and rows.data_ptr() == hseq.data_ptr()    # views, not copies
    d_w, d_b = W.xty_wide_reference(blocks, rows, head, shift, zero_row)
    want_w, want_b = GR.weight_grads(d_gi, d_gh_n, hseq, h0, done)
    torch.testing.assert_close(d_w, want_w, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(d_b, want_b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("in_f,out_f", [(64, 192), (256, 256), (128, 64)])
def test_backward_formula_equals_autograd(in_f, out_f):
    g = torch.Generator().manual_seed(in_f + out_f)
    x = torch.randn(5, 17, in_f, generator=g, dtype=torch.float64)
    w = torch.randn(out_f, in_f, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(out_f, generator=g, dtype=torch.float64, requires_grad=True)
    d_y = torch.randn(5, 17, out_f, generator=g, dtype=torch.float64)
    F.linear(x, w, b).backward(d_y)
    d_w, d_b = W.xty_wide_reference([d_y.reshape(-1, out_f)], x.reshape(-1, in_f))
    torch.testing.assert_close(d_w, w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(d_b, b.grad, rtol=1e-12, atol=1e-12)


def test_header_declares_the_entry_points_and_the_constants():
    src = open(HEADER).read()
    assert re.search(r"^int hftlob_xty_wide\(long long N, int Q, const float\* A0, int cols0, long long stride0, "
                     r"const float\* A1, int cols1,$", src, re.M)
    assert re.search(r"^long long hftlob_xty_wide_workspace\(long long N, int P, int Q\);", src, re.M)
    consts = dict(re.findall(r"^#define (HFTLOB_XTY_WIDE_[A-Z_]+) (\d+)", src, re.M))
    assert int(consts["HFTLOB_XTY_WIDE_MAX_P"]) == W.WIDE_MAX_P
    assert int(consts["HFTLOB_XTY_WIDE_TILE_P"]) == W.WIDE_TILE_P
    assert int(consts["HFTLOB_XTY_WIDE_CHUNK"]) == W.WIDE_CHUNK
    assert int(consts["HFTLOB_XTY_WIDE_STRIPE_ROWS"]) == W.WIDE_STRIPE_ROWS
    assert int(consts["HFTLOB_XTY_WIDE_TARGET_WGS"]) == W.WIDE_TARGET_WGS
    assert "hftlob_xty_wide" in _lib.EXPORTS and "hftlob_xty_wide_workspace" in _lib.EXPORTS


def test_stripe_rule():
    assert W.wide_max_stripes(768, 256) == 43 and W.wide_max_stripes(256, 256) == 128
    assert W.wide_max_stripes(64, 64) == 512 and W.wide_max_stripes(192, 64) == 256 and W.wide_max_stripes(64, 128) == 512
    for P, Q in ((768, 256), (256, 256), (64, 64), (192, 128)):
        M = W.wide_max_stripes(P, Q)
        assert W.wide_stripe_rule(0, P, Q) == (0, R)
        assert W.wide_stripe_rule(1, P, Q) == (1, R) and W.wide_stripe_rule(R, P, Q) == (1, R)
        assert W.wide_stripe_rule(R + 1, P, Q) == (2, R)
        assert W.wide_stripe_rule(M * R, P, Q) == (M, R)
        assert W.wide_stripe_rule(M * R + 1, P, Q) == (-(-(M * R + 1) // (R + 1)), R + 1)
        for N in (M * R + 1, 3 * M * R + 5, 10 ** 9):
            g, rows = W.wide_stripe_rule(N, P, Q)
            assert g <= M and (g - 1) * rows < N <= g * rows     # no stripe is empty, all rows are covered
    # the workload's shapes: at least two workgroups on each of 256 CUs
    for P, Q, tiles in ((768, 256, 12), (256, 256, 4)):
        assert W.wide_stripe_rule(65536, P, Q)[0] * tiles >= 512


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built")
    return _lib.lib()


@pytest.mark.parametrize("P,Q", [(64, 64), (192, 128), (256, 256), (768, 256)])
def test_workspace_size(L, P, Q):
    M, per = W.wide_max_stripes(P, Q), P * Q + P
    assert L.hftlob_xty_wide_workspace(0, P, Q) == 0 == W.wide_workspace_floats(0, P, Q)
    for N, stripes in ((1, 1), (R - 1, 1), (R, 1), (R + 1, 2), (M * R - 1, M), (M * R, M),
                       (M * R + 1, -(-(M * R + 1) // (R + 1))), (2 * M * R, M), (2 ** 33, M)):
        assert W.wide_stripe_rule(N, P, Q)[0] == stripes
        assert L.hftlob_xty_wide_workspace(N, P, Q) == stripes * per == W.wide_workspace_floats(N, P, Q)


def test_workspace_rejects_bad_sizes(L):
    for P in (0, 32, 65, 100, 832):
        assert L.hftlob_xty_wide_workspace(16, P, 64) == ESHAPE
    assert b"P must be" in L.hftlob_last_error()
    assert L.hftlob_xty_wide_workspace(16, 128, 96) == ESHAPE
    assert L.hftlob_xty_wide_workspace(-1, 128, 64) == ESHAPE
    assert b"N must be" in L.hftlob_last_error()


def test_xty_wide_rejects_bad_calls_before_any_device_work(L):
    k = C.c_void_p(64)   # never dereferenced: validation fails first
    bad = C.c_void_p(68)

    def X(N=16, Q=64, A0=k, cols0=128, stride0=128, A1=None, cols1=0, stride1=0, B=k, head=None, shift=0, zero_row=None,
          Cp=k, sum_a=None, ws=k):
        return L.hftlob_xty_wide(N, Q, A0, cols0, stride0, A1, cols1, stride1, B, head, shift, zero_row, Cp, sum_a, ws,
                                 None)

    # the shape, first of all (every pointer is bad as well)
    for kw in (dict(cols0=0), dict(cols0=96), dict(cols0=832), dict(cols1=32), dict(cols1=-64), dict(cols0=512, cols1=320),
               dict(Q=96), dict(N=-1), dict(shift=-1), dict(shift=17)):
        assert X(A0=None, B=bad, Cp=None, **kw) == ESHAPE, kw
    assert b"shift must be" in L.hftlob_last_error()
    assert X(Q=96) == ESHAPE and b"Q must be" in L.hftlob_last_error()
    # then the NULLs (with a misaligned pointer beside them)
    for kw in (dict(Cp=None), dict(A0=None), dict(cols1=64, stride1=64, A1=None), dict(B=None), dict(B=None, shift=15),
               dict(ws=None)):
        assert X(head=bad, **kw) == ENULL, kw
    assert b"null" in L.hftlob_last_error().lower()
    # then the alignment, the pointers before the strides
    for kw in (dict(A0=bad), dict(cols1=64, stride1=64, A1=bad), dict(B=bad), dict(head=bad, shift=4)):
        assert X(stride0=127, **kw) == EINVAL, kw
        assert b"16-byte aligned" in L.hftlob_last_error()
    for kw in (dict(stride0=127), dict(stride0=130), dict(cols1=64, A1=k, stride1=63), dict(cols1=64, A1=k, stride1=66)):
        assert X(**kw) == EINVAL, kw
        assert b"stride" in L.hftlob_last_error()
    # N = 0: C is still required (it is zero-filled), the shape is still checked, nothing else is looked at
    assert X(N=0, A0=None, B=None, ws=None, Cp=None) == ENULL
    assert X(N=0, Q=96, A0=None, B=None, ws=None) == ESHAPE
    assert X(N=0, shift=1, A0=None, B=None, ws=None) == ESHAPE


def test_wide_linear_supported_at_its_limits():
    S = W.wide_linear_supported
    for i in (64, 128, 256):
        assert all(S(i, o) for o in range(64, 769, 64))
        assert not S(i, 0) and not S(i, 32) and not S(i, 65) and not S(i, 832) and not S(i, 100)
    assert not S(96, 128) and not S(512, 128) and not S(32, 64) and not S(13, 256)
    assert W.WIDE_MAX_P == 768
    with pytest.raises(ValueError, match="not supported"):
        W.wide_linear(torch.zeros(3, 96), torch.zeros(128, 96))


def test_default_config_and_module_attribute():
    assert I.default_config()["FUSED_WGRAD_WIDE"] is False
    net = I.ActorCriticRNN(4, 3, 64, 64)
    assert net.fused_wgrad_wide is False and not any("fused" in k for k in net.state_dict())
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.fused_wgrad_wide = True
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


class _Space:
    def __init__(self, n=None, shape=None):
        self.n, self.shape = n, shape


class _MAC:
    number_of_agents_per_type = [1, 2]


class FakeEnv:
    """CPU stand-in with MARLEnv's interface (tests/test_ippo.py's, restated)."""
    device = torch.device("cpu")
    list_of_agents_configs = [object(), object()]
    multi_agent_config = _MAC()
    observation_spaces = [_Space(shape=(3,)), _Space(shape=(4,))]
    action_spaces = [_Space(n=3), _Space(n=2)]
    default_params = None

    def split_keys(self, keys, n):
        k = keys.to(torch.int64)
        j = torch.arange(n, dtype=torch.int64)
        return ((k[:, None, :] * 1_000_003 + j[None, :, None] * 7919 + 17) % (2 ** 31)).to(torch.int32)

    def reset(self, keys, params):
        E = keys.shape[0]
        self.t = torch.zeros(E, dtype=torch.int64)
        return [torch.zeros(E, 1, 3), torch.zeros(E, 2, 4)], None

    def step(self, keys, state, actions, params):
        E = keys.shape[0]
        self.t += 1
        done = self.t % 5 == 0
        r0 = (actions[0].view(E, 1) == 0).float()
        obs = [torch.randn(E, 1, 3), torch.randn(E, 2, 4)]
        dones = {"__all__": done, "agents": [done[:, None], done[:, None].repeat(1, 2)]}
        return obs, state, [r0, torch.zeros(E, 2)], dones, {}


def _cpu_config(**kw):
    return I.default_config(**dict(dict(NUM_ENVS=16, NUM_STEPS=10, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, NUM_MINIBATCHES=2,
                                        TOTAL_TIMESTEPS=16 * 10 * 4), **kw))


def test_trainer_switch_needs_a_gpu():
    with pytest.raises(ValueError, match="FUSED_WGRAD_WIDE needs a GPU device, got cpu"):
        I.IPPOTrainer(FakeEnv(), _cpu_config(FUSED_WGRAD_WIDE=True))
    tr = I.IPPOTrainer(FakeEnv(), _cpu_config())                  # the same config without the switch trains
    assert tr.fused_wgrad_wide is False and not any(n.fused_wgrad_wide for n in tr.nets)
    tr.update()


@pytest.mark.parametrize("hidden,fc", [(32, 64), (64, 96), (512, 64)])
def test_trainer_refuses_sizes_outside_the_set(hidden, fc, monkeypatch):
    """The sizes are checked at construction; the device check comes first, so the env claims a GPU (nothing
    is allocated there before the refusal)."""
    env = FakeEnv()
    monkeypatch.setattr(I.ActorCriticRNN, "to", lambda self, *a, **k: self)
    env.device = torch.device("cuda")
    with pytest.raises(ValueError, match="FUSED_WGRAD_WIDE needs GRU_HIDDEN_DIM and FC_DIM_SIZE in"):
        I.IPPOTrainer(env, _cpu_config(GRU_HIDDEN_DIM=hidden, FC_DIM_SIZE=fc, FUSED_WGRAD_WIDE=True))
