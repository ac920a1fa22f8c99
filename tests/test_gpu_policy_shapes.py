"""Every (FC, H) instantiation of the fused policy step (csrc/policy_step.hip: nine kernels per
operator, each with its own deal of column blocks over waves) on the GPU against the float64 CPU
restatement, at the cases of tests/policy_cases.py: a full obs tile (D = 64) with two tiles and one
live row, a ragged one (D = 61, four uneven heads) and saturated gates.  Tolerance, per tensor, the
project's own (tests/test_gpu_policy_step.py): |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|.  Actions
are compared exactly; tests/test_policy_cases_cpu.py checks on the CPU that every case's float64
top-two gap is >= 1e-3 and that float32 needs at most a quarter of the tolerance.

Sample keys have both words non-zero and the top bit set.  Every test is one or a few launches at
B <= 33; the references are computed once per case (policy_cases.case is cached)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_cases as PC
from hftlob import _lib
from hftlob.train import gru as G
from hftlob.train import ippo as I
from hftlob.train import policy as P
from test_gpu_policy_step import _abi_call, _sentinel_outputs, assert_close

pytestmark = pytest.mark.gpu

GAP = PC.GAP
TILE = 16
KEY0 = 0x9E3779B9
SAMPLED = [c for c in PC.CASES if c[0] in ("full", "ragged")]
NAMES = ("h", "action", "log_prob", "value", "logits")


def dev(d):
    return {k: v.cuda() for k, v in d.items()}


def key_words(k, k0=KEY0):
    return np.array([k0, (0xFFFFFFF0 + k) & 0xFFFFFFFF], np.uint32)


def key_tensor(k, k0=KEY0):
    return torch.from_numpy(key_words(k, k0).view(np.int32).copy()).cuda()


def noise(key, B, nvec):
    """The heads' Gumbel noise under ``key`` (split per head where there are several), float64 [B, S]."""
    return torch.cat([P.gumbel_noise(kk, B, n) for kk, n in zip(P.head_keys(key, len(nvec)), nvec)], -1).double()


def run(Wd, c, mode, nvec, flat, key=None, h=None, h_out=None, logits=True):
    """One launch: hftlob_policy_step where ``flat`` (one head, action [B]), else the multi-head operator."""
    h = c["h"] if h is None else h
    if flat:
        return P.policy_step(Wd, c["obs"], c["done"], h, mode, key=key, h_out=h_out, logits=logits)
    return P.policy_step_multi(Wd, c["obs"], c["done"], h, mode, nvec, key=key, h_out=h_out, logits=logits)


def picks(lg, score, nvec):
    """Per head the first argmax of score and the log-softmax of lg at it (float64): action [B, K], log_prob [B]."""
    acts, lp = [], 0.0
    for s, x in zip(score.split(list(nvec), -1), lg.split(list(nvec), -1)):
        acts.append(s.argmax(-1))
        lp = lp + torch.log_softmax(x, -1).gather(-1, acts[-1][:, None]).squeeze(-1)
    return torch.stack(acts, -1), lp


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_greedy_matches_float64(c):
    """full and saturated through hftlob_policy_step, ragged through hftlob_policy_step_multi; full again
    through the multi-head operator with one head (the NHD = 4 kernel of the pair), bit for bit."""
    kind = c[0]
    B, D, nvec, W, x, ref, info = PC.named_case(*c)
    print(f"{PC.case_id(c)}: top-two gap {info['gap']:.3e}, float32 CPU share of the bound {info['share']['max']:.4f}")
    assert info["gap"] >= GAP
    flat = len(nvec) == 1
    Wd, cd = dev(W), dev(x)
    h_out = torch.empty_like(cd["h"])
    _, action, log_prob, value, logits = run(Wd, cd, P.GREEDY, nvec, flat, h_out=h_out)
    assert_close("h", h_out, ref["h"])
    assert_close("logits", logits, ref["logits"])
    assert_close("value", value, ref["value"])
    assert_close("log_prob", log_prob, ref["log_prob"])
    assert action.dtype == torch.int32 and action.shape == ((B,) if flat else (B, len(nvec)))
    assert torch.equal(action.cpu().long().reshape(B, -1), ref["action"])
    assert torch.equal(cd["h"].cpu(), x["h"])                          # h_in is not touched when h_out is given
    for t in (h_out, logits, value, log_prob):
        assert bool(torch.isfinite(t).all())
    if kind == "full":
        multi = run(Wd, cd, P.GREEDY, nvec, False, h_out=torch.empty_like(cd["h"]))
        assert multi[1].shape == (B, 1)
        for name, a, b in zip(NAMES, (h_out, action, log_prob, value, logits),
                              (multi[0], multi[1][:, 0], multi[2], multi[3], multi[4])):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("c", SAMPLED, ids=PC.case_id)
def test_sampling_is_the_gumbel_argmax(c):
    kind = c[0]
    B, D, nvec, W, x, ref, _ = PC.named_case(*c)
    flat = len(nvec) == 1
    k = 0
    while PC.heads_gap(ref["logits"] + noise(key_words(k), B, nvec), nvec) < GAP:
        k += 1
        assert k < 64
    g = noise(key_words(k), B, nvec)
    Wd, cd = dev(W), dev(x)
    _, action, log_prob, value, logits = run(Wd, cd, P.SAMPLE, nvec, flat, key=key_tensor(k), h=cd["h"].clone())
    lg = logits.double().cpu()
    want, lp = picks(lg, lg + g, nvec)                                  # the GPU's own logits plus the host's noise
    greedy = picks(lg, lg, nvec)[0]
    print(f"key ({KEY0:#x}, {int(key_words(k)[1]):#x}); sampled != greedy on {int((want != greedy).sum())} of "
          f"{B * len(nvec)} draws")
    assert torch.equal(action.cpu().long().reshape(B, -1), want)       # every row of every head
    assert_close("log_prob", log_prob, lp)
    assert_close("logits", logits, ref["logits"])
    assert_close("value", value, ref["value"])
    ref_a = P.policy_step_multi_reference({kk: v.double() for kk, v in W.items()}, x["obs"].double(), x["done"],
                                          x["h"].double(), P.SAMPLE, nvec, key=key_words(k))[3]
    assert torch.equal(ref_a, want)                                    # the restatement from the key agrees
    if kind == "full":
        # only the key's first word changes: on the CPU the draw moves, so it must move on the GPU
        k0 = KEY0 ^ 0x80000001
        other = picks(ref["logits"], ref["logits"] + noise(key_words(k, k0), B, nvec), nvec)[0]
        assert not torch.equal(other, ref_a)
        got = run(Wd, cd, P.SAMPLE, nvec, flat, key=key_tensor(k, k0), h=cd["h"].clone(), logits=False)[1]
        assert not torch.equal(got, action), "the key's first word plays no part in the draw"


@pytest.mark.parametrize("FC,H", PC.PAIRS)
def test_in_place_changes_no_bit(FC, H):
    """h_out is h, at D = 64: with H = 64 the obs tile covers the whole LDS buffer that h is written
    into.  Both modes, logits = NULL in place."""
    B, D, nvec, W, x, _, _ = PC.named_case("full", FC, H)
    Wd, cd = dev(W), dev(x)
    for mode in (P.GREEDY, P.SAMPLE):
        key = key_tensor(5) if mode == P.SAMPLE else None
        sep = run(Wd, cd, mode, nvec, True, key=key, h_out=torch.empty_like(cd["h"]))
        h = cd["h"].clone()
        inp = run(Wd, cd, mode, nvec, True, key=key, h=h, logits=False)
        assert inp[0] is h and inp[4] is None
        for name, a, b in zip(NAMES[:4], sep[:4], inp[:4]):
            assert torch.equal(a, b), (mode, name)
        assert not torch.equal(h, cd["h"])


def _check_sentinels(B, S, bufs, names):
    for name, buf in zip(names, bufs):
        assert bool((buf[B:] == S).all()), f"{name}: rows past B were written"
        assert not bool((buf[:B] == S).any()), f"{name}: a live element was not written"


@pytest.mark.parametrize("mode", [P.GREEDY, P.SAMPLE])
@pytest.mark.parametrize("FC,H", [(64, 256), (256, 64)])
def test_rows_past_B_are_not_written(FC, H, mode):
    """B = 33: the third tile has one live row.  Every output has one spare tile of rows behind it,
    filled with a sentinel that must be intact afterwards (memory the test owns); through the C ABI."""
    B, D, nvec, W, x, ref, _ = PC.named_case("full", FC, H)
    S, A = -12345.0, nvec[0]
    Wd, cd = dev(W), dev(x)
    outs = _sentinel_outputs(B + TILE, H, A, S)
    _lib.check(_abi_call(Wd, cd, (B, D, FC, H, A), mode, key_tensor(3), outs))
    torch.cuda.synchronize()
    _check_sentinels(B, S, outs, ("h_out", "action", "log_prob", "value", "logits"))
    assert_close("h_out", outs[0][:B], ref["h"])
    assert_close("logits", outs[4][:B], ref["logits"])
    assert_close("value", outs[3][:B], ref["value"])
    if mode == P.GREEDY:
        assert torch.equal(outs[1][:B].cpu().long(), ref["action"][:, 0])
        assert_close("log_prob", outs[2][:B], ref["log_prob"])


def test_rows_past_B_are_not_written_multi_head():
    """hftlob_policy_step_multi through the C ABI at (FC, H) = (64, 256), B = 17, four uneven heads: the
    action rows are K words and the logits rows sum(nvec), each with a spare tile of sentinels behind."""
    FC, H = 64, 256
    B, D, nvec, W, x, ref, _ = PC.named_case("ragged", FC, H)
    S, K, A = -12345.0, len(nvec), sum(nvec)
    Wd, cd = dev(W), dev(x)
    rows = B + TILE
    f = lambda *s: torch.full(s, S, dtype=torch.float32, device="cuda")  # noqa: E731
    outs = [f(rows, H), torch.full((rows, K), int(S), dtype=torch.int32, device="cuda"), f(rows), f(rows), f(rows, A)]
    kk = 0
    while PC.heads_gap(ref["logits"] + noise(key_words(kk), B, nvec), nvec) < GAP:
        kk += 1
        assert kk < 64
    g = noise(key_words(kk), B, nvec)
    keys = torch.from_numpy(P.head_keys(key_words(kk), K).view(np.int32).copy()).cuda()   # [K, 2]: already split
    ws = P._weights_struct(Wd, D, FC, H, A)
    p = _lib.ptr
    for mode in (P.GREEDY, P.SAMPLE):
        for buf in outs:
            buf.fill_(S)
        _lib.check(_lib.lib().hftlob_policy_step_multi(
            B, D, FC, H, K, (C.c_int * K)(*nvec), C.byref(ws), p(cd["obs"]), p(cd["done"].view(torch.uint8)),
            p(cd["h"]), p(outs[0]), mode, p(keys), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]), _lib.stream_ptr()))
        torch.cuda.synchronize()
        _check_sentinels(B, S, outs, ("h_out", "action", "log_prob", "value", "logits"))
        assert_close("h_out", outs[0][:B], ref["h"])
        assert_close("logits", outs[4][:B], ref["logits"])
        assert_close("value", outs[3][:B], ref["value"])
        if mode == P.GREEDY:
            assert torch.equal(outs[1][:B].cpu().long(), ref["action"])
            assert_close("log_prob", outs[2][:B], ref["log_prob"])
        else:
            lg = outs[4][:B].double().cpu()
            want, lp = picks(lg, lg + g, nvec)
            assert torch.equal(outs[1][:B].cpu().long(), want)
            assert_close("log_prob", outs[2][:B], lp)


def test_all_done_ignores_the_carry():
    """(FC, H) = (128, 256) with every row done: h_in = 7.0 everywhere gives the bits of the case's h."""
    FC, H = 128, 256
    B, D, nvec, W, x, ref, info = PC.named_case("full", FC, H, done="all")
    assert bool(x["done"].all()) and info["gap"] >= GAP
    Wd, cd = dev(W), dev(x)
    for mode in (P.GREEDY, P.SAMPLE):
        key = key_tensor(7) if mode == P.SAMPLE else None
        own = run(Wd, cd, mode, nvec, True, key=key, h_out=torch.empty_like(cd["h"]))
        other = run(Wd, cd, mode, nvec, True, key=key, h=torch.full_like(cd["h"], 7.0))
        for name, a, b in zip(NAMES, own, other):
            assert torch.equal(a, b), (mode, name)
    assert_close("h", own[0], ref["h"])
    assert_close("logits", own[4], ref["logits"])
    assert_close("value", own[3], ref["value"])


@functools.lru_cache(maxsize=None)
def chain(FC, H, T=4, B=17):
    """T steps of the full case's net from its first B carries, with fresh obs and done per step (done on
    the odd rows at t = 0, then at rate 0.3): the float64 h of every step, and gi = relu(obs . w_embed^T
    + b_embed) . w_ih^T + b_ih in float64, rounded to float32 for the scan."""
    _, D, nvec, W, x, _, _ = PC.named_case("full", FC, H)
    g = torch.Generator().manual_seed(1000 + FC + 3 * H)
    obs = torch.randn(T, B, D, generator=g, dtype=torch.float32)
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = torch.arange(B) % 2 == 1
    h0 = x["h"][:B].clone()
    Wd = {k: v.double() for k, v in W.items()}
    h, hs = h0.double(), []
    for t in range(T):
        h = P.policy_step_multi_reference(Wd, obs[t].double(), done[t], h, P.GREEDY, nvec)[0]
        hs.append(h)
    gi = torch.relu(obs.double() @ Wd["w_embed"].t() + Wd["b_embed"]) @ Wd["w_ih"].t() + Wd["b_ih"]
    return W, obs, done, h0, torch.stack(hs), gi.float()


@pytest.mark.parametrize("FC,H", [(128, 256), (256, 128)])
def test_rollout_recurrence_is_the_updates_recurrence(FC, H):
    """The carry chained through T policy steps (the rollout) and the GRU scan over the same inputs (the
    update) are the same recurrence: both within the bound of the float64 chain, and within twice the
    bound of each other."""
    W, obs, done, h0, href, gi = chain(FC, H)
    T, B = done.shape
    Wd = dev(W)
    h, hs = h0.cuda(), []
    for t in range(T):
        h = P.policy_step(Wd, obs[t].cuda(), done[t].cuda(), h, P.GREEDY, h_out=torch.empty_like(h))[0]
        hs.append(h)
    stepped = torch.stack(hs)
    scanned, _ = G.scan_forward(gi.cuda(), h0.cuda(), done.cuda(), Wd["w_hh"], Wd["b_hh"], save_gates=False)
    assert_close("h, stepped", stepped, href)
    assert_close("h, scanned", scanned, href)
    bound = 1e-5 * href.abs() + 1e-5 * float(href.abs().max())
    worst = float(((stepped.double().cpu() - scanned.double().cpu()).abs() / (2.0 * bound)).max())
    print(f"h, stepped against scanned: max difference / twice the bound = {worst:.4f}")
    assert worst <= 1.0


def test_module_step():
    """policy_step_net on an ActorCriticRNN with FC 256, H 128 and four uneven heads at D = 61, against
    net.step in torch on the GPU."""
    nvec = [3, 16, 1, 5]
    torch.manual_seed(0)
    net = I.ActorCriticRNN(61, nvec, 256, 128).cuda()
    g = torch.Generator().manual_seed(1)
    B = 24
    obs, h = torch.randn(B, 61, generator=g).cuda(), torch.randn(B, 128, generator=g).cuda()
    done = (torch.arange(B) % 2 == 1).cuda()
    with torch.no_grad():
        h1, logits, v = net.step(h, obs, done)
    out = P.policy_step_multi(net, obs, done, h.clone(), P.GREEDY, nvec, logits=True)
    assert_close("h", out[0], h1)
    assert_close("logits", out[4], logits)
    assert_close("value", out[3], v)
    lg = out[4].double().cpu()
    want, lp = picks(lg, lg, nvec)
    assert torch.equal(out[1].cpu().long(), want)
    assert_close("log_prob", out[2], lp)
    hh = h.clone()
    res = P.policy_step_net(net, obs, done, hh, P.GREEDY)              # the operator the net's heads need, in place
    assert res[0] is hh and res[4] is None and res[1].shape == (B, 4)
    for name, a, b in zip(NAMES[:4], res[:4], out[:4]):
        assert torch.equal(a, b), name
