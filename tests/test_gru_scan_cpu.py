"""The fused GRU scan without a GPU: the torch restatement of the two operators
(hftlob.train.gru) against autograd through ActorCriticRNN.forward's loop in float64, the
C-ABI surface of hftlob_gru_scan_fwd / _bwd (declared, exported, argument checks before any
device call), and the learner's FUSED_GRU switch."""
import ctypes as C
import os
import re

import pytest
import torch

from hftlob import _lib
from hftlob.train import gru as G
from hftlob.train import ippo as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")


def make_case(T, B, H, seed, all_done_t0=False, dtype=torch.float64):
    """Random scan inputs: done at rate 0.3 with every second row (or every row) done at t = 0."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).to(dtype)  # noqa: E731
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = True if all_done_t0 else (torch.arange(B) % 2 == 1)
    return dict(gi=r(T, B, 3 * H), h0=r(B, H), done=done, w_hh=r(3 * H, H) / H ** 0.5, b_hh=0.5 * r(3 * H),
                d_hseq=r(T, B, H))


def loop_autograd(c):
    """The scan of ActorCriticRNN.forward (its loop, on an nn.GRUCell's weight_hh / bias_hh) with
    autograd: (hseq, d_gi, d_h0, d_w_hh, d_b_hh) for the cotangent d_hseq."""
    T, B, H3 = c["gi"].shape
    cell = torch.nn.GRUCell(4, H3 // 3).to(c["gi"].dtype)
    with torch.no_grad():
        cell.weight_hh.copy_(c["w_hh"])
        cell.bias_hh.copy_(c["b_hh"])
    gi_all = c["gi"].clone().requires_grad_(True)
    h0 = c["h0"].clone().requires_grad_(True)
    w_hh, b_hh = cell.weight_hh, cell.bias_hh
    hseq = I.ActorCriticRNN.scan_loop(gi_all, h0, c["done"], w_hh, b_hh)
    hseq.backward(c["d_hseq"])
    return hseq.detach(), gi_all.grad, h0.grad, w_hh.grad, b_hh.grad


@pytest.mark.parametrize("T,B,H,all0", [(1, 1, 64, False), (5, 17, 64, False), (8, 33, 256, False),
                                        (4, 6, 64, True)])
def test_restatement_matches_autograd_float64(T, B, H, all0):
    c = make_case(T, B, H, seed=T * 1000 + B, all_done_t0=all0)
    want = loop_autograd(c)
    hseq, gates = G.gru_scan_reference(c["gi"], c["h0"], c["done"], c["w_hh"], c["b_hh"])
    d_gi, d_gh_n, d_h0 = G.gru_scan_backward_reference(c["d_hseq"], hseq, gates, c["h0"], c["done"], c["w_hh"])
    d_w, d_b = G.weight_grads(d_gi, d_gh_n, hseq, c["h0"], c["done"])
    assert gates.shape == (T, B, 4 * H) and d_gh_n.shape == (T, B, H)
    for name, got, ref in zip(("hseq", "d_gi", "d_h0", "d_w_hh", "d_b_hh"), (hseq, d_gi, d_h0, d_w, d_b), want):
        err = float((got - ref).abs().max())
        assert err <= 1e-12, (name, err)
    if all0:
        assert torch.equal(d_h0, torch.zeros_like(d_h0))


def test_abi_surface_and_argument_checks():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(hftlob_[a-z_]+)\s*\(", src))
    for name in ("hftlob_gru_scan_fwd", "hftlob_gru_scan_bwd"):
        assert name in declared and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8 and "#define HFTLOB_ABI_VERSION 8" in src
    assert not G.gru_scan_supported(32) and not G.gru_scan_supported(96)
    assert all(G.gru_scan_supported(h) for h in (64, 128, 256))
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    assert L.hftlob_version() == 8
    k = C.c_void_p(64)   # never dereferenced: the checks run on the host before any device call
    fwd, bwd = L.hftlob_gru_scan_fwd, L.hftlob_gru_scan_bwd
    ENULL, ESHAPE = -2, -3
    good_f, good_b = [k] * 6 + [None], [k] * 9        # forward: gates may be NULL
    for i in range(6):                                # every other forward pointer is required
        a = list(good_f)
        a[i] = None
        assert fwd(4, 8, 64, *a, None) == ENULL, i
        assert b"null" in L.hftlob_last_error()
    for i in range(9):
        a = list(good_b)
        a[i] = None
        assert bwd(4, 8, 64, *a, None) == ENULL, i
    for H in (32, 96, 0, 512):
        assert fwd(4, 8, H, *good_f, None) == ESHAPE and bwd(4, 8, H, *good_b, None) == ESHAPE
        assert b"H must be" in L.hftlob_last_error()
    for T, B in ((0, 8), (4, 0), (-1, 8), (4, -1)):
        assert fwd(T, B, 64, *good_f, None) == ESHAPE and bwd(T, B, 64, *good_b, None) == ESHAPE
    with pytest.raises(RuntimeError, match="device"):   # a CPU tensor raises through _lib.ptr
        c = make_case(2, 3, 64, 0, dtype=torch.float32)
        G.gru_scan(c["gi"], c["h0"], c["done"], c["w_hh"], c["b_hh"])


def test_config_switch():
    from test_ippo import FakeEnv
    assert I.default_config()["FUSED_GRU"] is False
    kw = dict(NUM_ENVS=16, NUM_STEPS=4, FC_DIM_SIZE=16, NUM_MINIBATCHES=2, UPDATE_EPOCHS=1,
              TOTAL_TIMESTEPS=16 * 4 * 4, SEED=0)
    with pytest.raises(ValueError, match=r"FUSED_GRU needs GRU_HIDDEN_DIM in \[64, 128, 256\]"):
        I.IPPOTrainer(FakeEnv(), I.default_config(GRU_HIDDEN_DIM=16, FUSED_GRU=True, **kw))
    off = I.IPPOTrainer(FakeEnv(), I.default_config(GRU_HIDDEN_DIM=16, **kw))
    assert not any(n.fused for n in off.nets)
    cpu = I.IPPOTrainer(FakeEnv(), I.default_config(GRU_HIDDEN_DIM=64, FUSED_GRU=True, **kw))
    assert not any(n.fused for n in cpu.nets)          # a supported size on the CPU: the loop
    cpu.update()
