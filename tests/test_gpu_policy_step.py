"""The fused policy step on the GPU (hftlob_policy_step, hftlob.train.policy.policy_step) against
the float64 CPU restatement evaluated from the same float32 inputs.  Tolerance, per tensor, the
project's own (tests/test_gpu_gru_scan.py): |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, and exactly 0
where the whole reference tensor is 0.  Actions are compared exactly, after the test has checked on
the CPU that the float64 top-two gap of every row is >= 1e-3 (a float32 sum of this size carries
about 1e-6 of error)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.train import ippo as I
from hftlob.train import policy as P

pytestmark = pytest.mark.gpu

# (B, D, FC, H, A, every row done): one row, D no multiple of 4; exactly one tile; a second tile with
# one live row, FC != H; H > FC and a full action block; the learner's sizes, every k loop at full
# length; that again with every carry reset; a head of one logit (action 0, log-prob exactly 0), one
# tile plus one row at the smallest D and the smallest kernel
CASES = [(1, 3, 64, 64, 2, False), (16, 6, 64, 64, 5, False), (17, 13, 128, 64, 10, False),
         (33, 16, 64, 128, 16, False), (40, 9, 256, 256, 9, False), (40, 9, 256, 256, 9, True),
         (17, 1, 64, 64, 1, False)]
TILE = 16
GAP = 1e-3


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


def top_two_gap(score):
    if score.shape[-1] < 2:                                            # a one-logit head has no second
        return float("inf")
    top = score.double().topk(2, dim=-1).values
    return float((top[:, 0] - top[:, 1]).min())


@functools.lru_cache(maxsize=None)
def case(B, D, FC, H, A, all_done):
    """Float32 weights (randn / sqrt(fan_in), non-zero biases, w_a2 at gain 1) and inputs (done on the
    odd rows, or everywhere), and the float64 CPU reference of mode 1; computed once per shape and not
    modified by the tests."""
    g = torch.Generator().manual_seed(11 * B + 5 * D + FC + 3 * H + A)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    lin = lambda o, i: (r(o, i) / i ** 0.5, 0.5 * r(o))  # noqa: E731
    W = {}
    for name, o, i in (("embed", FC, D), ("ih", 3 * H, FC), ("hh", 3 * H, H), ("c1", FC, H), ("c2", 1, FC),
                       ("a1", H, H), ("a2", A, H)):
        W["w_" + name], W["b_" + name] = lin(o, i)
    done = torch.ones(B, dtype=torch.bool) if all_done else torch.arange(B) % 2 == 1
    x = dict(obs=r(B, D), h=r(B, H), done=done)
    ref = P.policy_step_reference({k: v.double() for k, v in W.items()}, x["obs"].double(), done, x["h"].double(),
                                  P.GREEDY)
    return W, x, dict(zip(("h", "logits", "value", "action", "log_prob"), ref))


def dev(d):
    return {k: v.cuda() for k, v in d.items()}


def key_tensor(k):
    return torch.tensor([0, k], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("B,D,FC,H,A,all_done", CASES)
def test_outputs_match_float64(B, D, FC, H, A, all_done):
    W, x, ref = case(B, D, FC, H, A, all_done)
    gap = top_two_gap(ref["logits"])
    print(f"smallest float64 top-two logit gap = {gap:.3e}")
    assert gap >= GAP, "pick another seed: a row's two largest logits are too close for exact actions"
    Wd, c = dev(W), dev(x)
    h_out = torch.empty_like(c["h"])
    _, action, log_prob, value, logits = P.policy_step(Wd, c["obs"], c["done"], c["h"], P.GREEDY, h_out=h_out,
                                                       logits=True)
    assert_close("h", h_out, ref["h"])
    assert_close("logits", logits, ref["logits"])
    assert_close("value", value, ref["value"])
    assert action.dtype == torch.int32 and torch.equal(action.cpu().long(), ref["action"])
    assert_close("log_prob", log_prob, ref["log_prob"])
    if A == 1:
        assert not bool(action.any()) and bool((log_prob == 0.0).all())
    assert torch.equal(c["h"].cpu(), x["h"])                           # h_in is not touched when h_out is given
    if all_done:                                                       # the carry plays no part
        other = P.policy_step(Wd, c["obs"], c["done"], torch.full_like(c["h"], 7.0), P.GREEDY, logits=True)
        assert torch.equal(other[0], h_out) and torch.equal(other[4], logits)


@pytest.mark.parametrize("B,D,FC,H,A,all_done", [CASES[1], CASES[4]])
def test_exact_ties_take_the_first(B, D, FC, H, A, all_done):
    W, x, _ = case(B, D, FC, H, A, all_done)
    W = {k: v.clone() for k, v in W.items()}
    W["w_a2"][3] = W["w_a2"][1]
    W["b_a2"][1] = W["b_a2"][3] = 50.0                                 # both beat the rest, and tie exactly
    c = dev(x)
    out = P.policy_step(dev(W), c["obs"], c["done"], c["h"].clone(), P.GREEDY, logits=True)
    assert bool((out[4][:, 1] == out[4][:, 3]).all()) and bool((out[4][:, 1] > 40).all())
    assert out[1].tolist() == [1] * B


@pytest.mark.parametrize("B,D,FC,H,A,all_done", CASES[:5] + CASES[6:])
def test_sampling_is_the_gumbel_argmax(B, D, FC, H, A, all_done):
    W, x, ref = case(B, D, FC, H, A, all_done)
    k = 0
    while top_two_gap(ref["logits"] + P.gumbel_noise(np.array([0, k], np.uint32), B, A).double()) < GAP:
        k += 1
        assert k < 64
    g = P.gumbel_noise(np.array([0, k], np.uint32), B, A).double()
    Wd, c = dev(W), dev(x)
    _, action, log_prob, value, logits = P.policy_step(Wd, c["obs"], c["done"], c["h"].clone(), P.SAMPLE,
                                                       key=key_tensor(k), logits=True)
    lg = logits.double().cpu()
    want = (lg + g).argmax(-1)
    print(f"key (0, {k}); sampled != greedy on {int((want != lg.argmax(-1)).sum())} of {B} rows")
    assert torch.equal(action.cpu().long(), want)                      # every row
    assert_close("log_prob", log_prob, torch.log_softmax(lg, -1).gather(-1, want[:, None]).squeeze(-1))
    assert_close("value", value, ref["value"])
    if A == 1:
        assert not bool(action.any()) and bool((log_prob == 0.0).all())
    if B == 40:
        other = P.policy_step(Wd, c["obs"], c["done"], c["h"].clone(), P.SAMPLE, key=key_tensor(k + 1))[1]
        assert not torch.equal(other, action)


def test_host_noise_is_the_oracles_bits():
    from oracle import ref_py as R
    for key, B, A in (((0, 100), 17, 16), ((7, 0xFFFFFFF0), 40, 10)):
        bits = R.random_bits(key, B * A, True)
        assert P.random_bits(np.array(key, np.uint32), B * A).tolist() == bits
        want = P.gumbel_from_bits(np.array(bits, dtype=np.uint32)).reshape(B, A)
        assert np.array_equal(P.gumbel_noise(np.array(key, np.uint32), B, A).numpy(), want)


@pytest.mark.parametrize("mode", [P.GREEDY, P.SAMPLE])
def test_in_place_and_null_logits_change_no_bit(mode):
    W, x, _ = case(*CASES[2])
    Wd, c = dev(W), dev(x)
    key = key_tensor(5) if mode == P.SAMPLE else None
    sep = P.policy_step(Wd, c["obs"], c["done"], c["h"], mode, key=key, h_out=torch.empty_like(c["h"]), logits=True)
    h = c["h"].clone()
    inp = P.policy_step(Wd, c["obs"], c["done"], h, mode, key=key)     # in place, logits = NULL
    assert inp[0] is h and inp[4] is None
    for name, a, b in zip(("h", "action", "log_prob", "value"), sep[:4], inp[:4]):
        assert torch.equal(a, b), name


def _abi_call(Wd, c, sizes, mode, key, outs, logits=True, **over):
    """hftlob_policy_step through the C ABI on the tensors of ``outs`` (h_out, action, log_prob, value,
    logits); ``over`` replaces arguments by name."""
    B, D, FC, H, A = sizes
    ws = P._weights_struct(Wd, D, FC, H, A)
    p = _lib.ptr
    a = dict(B=B, D=D, FC=FC, H=H, A=A, w=C.byref(ws), obs=p(c["obs"]), done=p(c["done"].view(torch.uint8)),
             h_in=p(c["h"]), h_out=p(outs[0]), mode=mode, key=p(key), action=p(outs[1]), log_prob=p(outs[2]),
             value=p(outs[3]), logits=p(outs[4]) if logits else None)
    a.update(over)
    return _lib.lib().hftlob_policy_step(a["B"], a["D"], a["FC"], a["H"], a["A"], a["w"], a["obs"], a["done"],
                                         a["h_in"], a["h_out"], a["mode"], a["key"], a["action"], a["log_prob"],
                                         a["value"], a["logits"], _lib.stream_ptr())


def _sentinel_outputs(rows, H, A, S):
    f = lambda *s: torch.full(s, S, dtype=torch.float32, device="cuda")  # noqa: E731
    return [f(rows, H), torch.full((rows,), int(S), dtype=torch.int32, device="cuda"), f(rows), f(rows), f(rows, A)]


@pytest.mark.parametrize("mode", [P.GREEDY, P.SAMPLE])
def test_rows_past_B_are_not_written(mode):
    """B = 17: the second tile has one live row.  Every output has one spare tile of rows behind it,
    filled with a sentinel that must be intact afterwards (memory the test owns)."""
    B, D, FC, H, A, _ = CASES[2]
    S = -12345.0
    W, x, ref = case(*CASES[2])
    Wd, c = dev(W), dev(x)
    outs = _sentinel_outputs(B + TILE, H, A, S)
    _lib.check(_abi_call(Wd, c, (B, D, FC, H, A), mode, key_tensor(3), outs))
    torch.cuda.synchronize()
    for name, buf in zip(("h_out", "action", "log_prob", "value", "logits"), outs):
        assert bool((buf[B:] == S).all()), f"{name}: rows past B were written"
        assert not bool((buf[:B] == S).any()), f"{name}: a live element was not written"
    assert_close("h_out", outs[0][:B], ref["h"])
    assert_close("logits", outs[4][:B], ref["logits"])
    assert_close("value", outs[3][:B], ref["value"])


def test_error_codes_launch_nothing():
    B, D, FC, H, A, _ = CASES[1]
    S = -12345.0
    W, x, _ = case(*CASES[1])
    Wd, c = dev(W), dev(x)
    outs = _sentinel_outputs(B, H, A, S)
    L = _lib.lib()
    EINVAL, ENULL, ESHAPE = -1, -2, -3
    for over, mode, key, code, word in ((dict(H=96), 1, None, ESHAPE, b"H"), (dict(A=17), 1, None, ESHAPE, b"A"),
                                        (dict(D=0), 1, None, ESHAPE, b"D"), (dict(mode=2), 1, None, EINVAL, b"mode"),
                                        (dict(obs=None), 1, None, ENULL, b"obs"), ({}, 0, None, ENULL, b"key")):
        mode = over.pop("mode", mode)
        assert _abi_call(Wd, c, (B, D, FC, H, A), mode, key, outs, **over) == code, (over, mode)
        assert word in L.hftlob_last_error(), (over, L.hftlob_last_error())
    torch.cuda.synchronize()
    for buf in outs:
        assert bool((buf == S).all())
    assert _abi_call(Wd, c, (B, D, FC, H, A), 1, None, outs) == 0          # the same call with good arguments runs
    torch.cuda.synchronize()
    assert not any(bool((buf == S).any()) for buf in outs)


def test_captures_and_replays_bit_for_bit():
    """One mode-0 call inside a torch.cuda.graph (warm-up on a side stream); two replays with new obs,
    done, h and key contents equal the eager call bit for bit."""
    B, D, FC, H, A, _ = CASES[2]
    W, x, _ = case(*CASES[2])
    Wd = dev(W)
    st = dev(x)
    st["h"] = st["h"].clone()
    key = key_tensor(0)
    h_out = torch.empty_like(st["h"])
    out = tuple(torch.empty(B, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.float32))
    run = lambda: P.policy_step(Wd, st["obs"], st["done"], st["h"], P.SAMPLE, key=key, out=out, h_out=h_out)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    g = torch.Generator().manual_seed(1)
    seen = []
    for rep in range(2):
        new = dict(obs=torch.randn(B, D, generator=g).cuda(), h=torch.randn(B, H, generator=g).cuda(),
                   done=(torch.rand(B, generator=g) < 0.5).cuda())
        for k, v in new.items():
            st[k].copy_(v)
        key.copy_(key_tensor(17 + rep))
        graph.replay()
        torch.cuda.synchronize()
        got = [h_out.clone()] + [o.clone() for o in out]
        eager = P.policy_step(Wd, new["obs"], new["done"], new["h"], P.SAMPLE, key=key_tensor(17 + rep),
                              h_out=torch.empty_like(new["h"]))
        for name, a, b in zip(("h", "action", "log_prob", "value"), got, eager[:4]):
            assert torch.equal(a, b), (rep, name)
        seen.append(got[1])
    assert not torch.equal(seen[0], seen[1])


def test_module_step():
    torch.manual_seed(0)
    net = I.ActorCriticRNN(6, 5, 64, 64).cuda()
    g = torch.Generator().manual_seed(1)
    B = 24
    obs, h = torch.randn(B, 6, generator=g).cuda(), torch.randn(B, 64, generator=g).cuda()
    done = (torch.arange(B) % 2 == 1).cuda()
    with torch.no_grad():
        h1, logits, v = net.step(h, obs, done)
    out = P.policy_step(net, obs, done, h.clone(), P.GREEDY, logits=True)
    assert_close("h", out[0], h1)
    assert_close("logits", out[4], logits)
    assert_close("value", out[3], v)
    lp = torch.log_softmax(out[4].double(), -1).gather(-1, out[1].long()[:, None]).squeeze(-1)
    assert_close("log_prob", out[2], lp)
    a, lpb, vb = (torch.empty(B, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.float32))
    hh = h.clone()
    res = P.policy_step(net, obs, done, hh, P.GREEDY, out=(a, lpb, vb))    # the caller's tensors, the carry in place
    assert res[0] is hh and res[1] is a and torch.equal(hh, out[0]) and torch.equal(a, out[1])
    assert torch.equal(lpb, out[2]) and torch.equal(vb, out[3])
    with pytest.raises(ValueError, match="policy_step needs"):
        P.policy_step(I.ActorCriticRNN(6, 5, 64, 32).cuda(), obs, done, torch.zeros(B, 32, device="cuda"), P.GREEDY)
    with pytest.raises(ValueError, match="mode 0 needs key"):
        P.policy_step(net, obs, done, h.clone(), P.SAMPLE)
