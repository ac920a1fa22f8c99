"""The narrow layers' weight gradient without a GPU: the torch restatement (hftlob.train.wgrad.xty_reference)
and the backward formulas of narrow_linear against float64 autograd, the header's constants and
declarations, the argument checks of hftlob_xty / hftlob_xty_workspace on the built library (they run
before any device work), narrow_linear_supported at its limits and the trainer's FUSED_WGRAD switch on a
CPU device."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from hftlob import _lib
from hftlob.train import ippo as I
from hftlob.train import wgrad as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")
OK, EINVAL, ENULL, ESHAPE = 0, -1, -2, -3
R, G = W.STRIPE_ROWS, W.MAX_STRIPES


@pytest.mark.parametrize("N,P,Q", [(1, 1, 64), (1, 13, 256), (7, 1, 128), (33, 10, 64), (130, 64, 256)])
def test_reference_is_the_transposed_product_and_the_column_sums(N, P, Q):
    g = torch.Generator().manual_seed(N + P)
    A = torch.randn(N, P, generator=g, dtype=torch.float64)
    B = torch.randn(N, Q, generator=g, dtype=torch.float64)
    c, sa, sb = W.xty_reference(A, B)
    assert c.dtype == torch.float64 and c.shape == (P, Q) and sa.shape == (P,) and sb.shape == (Q,)
    want = torch.zeros(P, Q, dtype=torch.float64)
    for n in range(N):
        want += A[n][:, None] * B[n][None, :]
    torch.testing.assert_close(c, want, rtol=1e-12, atol=1e-12)
    assert torch.equal(c, A.T @ B)
    torch.testing.assert_close(sa, A.sum(0), rtol=0, atol=0)
    torch.testing.assert_close(sb, B.sum(0), rtol=0, atol=0)


@pytest.mark.parametrize("in_f,out_f", [(64, 13), (128, 1), (12, 64), (2, 256), (64, 64)])
def test_backward_formulas_equal_autograd(in_f, out_f):
    """d_w and d_b of F.linear from xty_reference, in the orientation narrow_linear picks for the layer."""
    g = torch.Generator().manual_seed(in_f + out_f)
    x = torch.randn(5, 17, in_f, generator=g, dtype=torch.float64)
    w = torch.randn(out_f, in_f, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(out_f, generator=g, dtype=torch.float64, requires_grad=True)
    d_y = torch.randn(5, 17, out_f, generator=g, dtype=torch.float64)
    F.linear(x, w, b).backward(d_y)
    x2, d2 = x.reshape(-1, in_f), d_y.reshape(-1, out_f)
    if 1 <= out_f <= W.MAX_P and in_f in W.SUPPORTED_Q:      # narrow output: A = d_y, B = x
        d_w, d_b, _ = W.xty_reference(d2, x2)
    else:                                                     # narrow input: A = x, B = d_y
        c, _, d_b = W.xty_reference(x2, d2)
        d_w = c.t()
    torch.testing.assert_close(d_w, w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(d_b, b.grad, rtol=1e-12, atol=1e-12)


def test_header_declares_the_entry_points_and_the_constants():
    src = open(HEADER).read()
    assert re.search(r"^int hftlob_xty\(long long N, int P, int Q, const float\* A", src, re.M)
    assert re.search(r"^long long hftlob_xty_workspace\(long long N, int P, int Q\);", src, re.M)
    consts = dict(re.findall(r"^#define (HFTLOB_XTY_[A-Z_]+) (\d+)", src, re.M))
    assert int(consts["HFTLOB_XTY_STRIPE_ROWS"]) == W.STRIPE_ROWS
    assert int(consts["HFTLOB_XTY_MAX_STRIPES"]) == W.MAX_STRIPES
    assert int(consts["HFTLOB_XTY_MAX_P"]) == W.MAX_P
    assert re.search(r"^#define HFTLOB_ABI_VERSION 8$", src, re.M) and _lib.ABI_VERSION == 8
    assert "hftlob_xty" in _lib.EXPORTS and "hftlob_xty_workspace" in _lib.EXPORTS


def test_stripe_rule():
    assert W.stripe_rule(0) == (0, R)
    assert W.stripe_rule(1) == (1, R) and W.stripe_rule(R) == (1, R) and W.stripe_rule(R + 1) == (2, R)
    assert W.stripe_rule(G * R) == (G, R)
    assert W.stripe_rule(G * R + 1) == (-(-(G * R + 1) // (R + 1)), R + 1)
    for N in (G * R + 1, 3 * G * R + 5, 10 ** 9):
        g, rows = W.stripe_rule(N)
        assert g <= G and (g - 1) * rows < N <= g * rows     # no stripe is empty, all rows are covered


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built")
    return _lib.lib()


def test_library_keeps_the_abi_version(L):
    assert L.hftlob_version() == 8


@pytest.mark.parametrize("P,Q", [(1, 64), (13, 256), (64, 128)])
def test_workspace_size(L, P, Q):
    per = P * Q + P + Q
    assert L.hftlob_xty_workspace(0, P, Q) == 0
    for N, stripes in ((1, 1), (R - 1, 1), (R, 1), (R + 1, 2), (G * R - 1, G), (G * R, G),
                       (G * R + 1, -(-(G * R + 1) // (R + 1))), (2 * G * R, G), (2 ** 33, G)):
        assert W.stripe_rule(N)[0] == stripes
        assert L.hftlob_xty_workspace(N, P, Q) == stripes * per == W.workspace_floats(N, P, Q)


def test_workspace_rejects_bad_sizes(L):
    assert L.hftlob_xty_workspace(16, 0, 64) == ESHAPE
    assert L.hftlob_xty_workspace(16, 65, 64) == ESHAPE
    assert L.hftlob_xty_workspace(16, 13, 96) == ESHAPE
    assert L.hftlob_xty_workspace(-1, 13, 64) == ESHAPE
    assert b"N must be" in L.hftlob_last_error()


def test_xty_rejects_bad_calls_before_any_device_work(L):
    k = C.c_void_p(64)   # never dereferenced: validation fails first
    X = L.hftlob_xty
    assert X(16, 0, 64, k, k, k, None, None, k, None) == ESHAPE
    assert X(16, 65, 64, k, k, k, None, None, k, None) == ESHAPE
    assert X(16, 13, 96, k, k, k, None, None, k, None) == ESHAPE
    assert b"Q must be" in L.hftlob_last_error()
    assert X(-1, 13, 64, k, k, k, None, None, k, None) == ESHAPE
    assert X(16, 13, 64, None, k, k, None, None, k, None) == ENULL
    assert X(16, 13, 64, k, None, k, None, None, k, None) == ENULL
    assert X(16, 13, 64, k, k, None, None, None, k, None) == ENULL
    assert X(16, 13, 64, k, k, k, None, None, None, None) == ENULL
    assert b"null" in L.hftlob_last_error().lower()
    assert X(16, 13, 64, k, C.c_void_p(68), k, None, None, k, None) == EINVAL       # B not 16-byte aligned
    # N = 0: C is still required (it is zero-filled); A, B and the workspace are not looked at
    assert X(0, 13, 64, None, None, None, None, None, None, None) == ENULL
    assert X(0, 13, 96, None, None, k, None, None, None, None) == ESHAPE


def test_narrow_linear_supported_at_its_limits():
    S = W.narrow_linear_supported
    for wide in (64, 128, 256):
        assert S(wide, 1) and S(wide, 64) and S(1, wide) and S(64, wide)
        assert not S(wide, 0) and not S(0, wide)
    assert S(256, 65) is False and S(65, 256) is False       # the narrow side past MAX_P (and 65 is no wide side)
    assert not S(96, 13) and not S(13, 96) and not S(32, 13) and not S(13, 512) and not S(512, 13)
    assert S(64, 64) and S(128, 64) and S(64, 128)            # narrow on both sides, or a wide side <= MAX_P
    assert not S(128, 128) and not S(256, 256)                # the square layers stay with rocBLAS
    assert W.MAX_P == 64 and W.SUPPORTED_Q == (64, 128, 256)


def test_narrow_linear_refuses_an_unsupported_layer():
    with pytest.raises(ValueError, match="not supported"):
        W.narrow_linear(torch.zeros(3, 256), torch.zeros(256, 256))


def test_default_config_and_module_attribute():
    assert I.default_config()["FUSED_WGRAD"] is False
    net = I.ActorCriticRNN(4, 3, 16, 16)
    assert net.fused_wgrad is False and "fused_wgrad" not in net.state_dict()


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


def test_trainer_switch_needs_a_gpu():
    c = I.default_config(NUM_ENVS=16, NUM_STEPS=10, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, NUM_MINIBATCHES=2,
                         TOTAL_TIMESTEPS=16 * 10 * 4, FUSED_WGRAD=True)
    with pytest.raises(ValueError, match="FUSED_WGRAD needs a GPU device, got cpu"):
        I.IPPOTrainer(FakeEnv(), c)
    tr = I.IPPOTrainer(FakeEnv(), dict(c, FUSED_WGRAD=False))     # the same config without the switch trains
    assert tr.fused_wgrad is False and not any(n.fused_wgrad for n in tr.nets)
    tr.update()
