"""The training diagnostics (TRAIN_DIAG) without a GPU: the two new entry points' ABI and argument checks, the
torch definitions (``rollout_diag_reference`` against exact counts and ``math.fsum``, ``world_tally_reference``
against a plain double loop), ``TrainDiag`` on hand-made tensors, and the CPU trainer and a two-member population
on a stand-in env that fills ``last_rewards`` and ``last_info_words``: training is bit for bit what it is without
the switch, and the diagnostics are ``reduce_steps`` over the steps the env recorded."""
import ctypes as C
import dataclasses
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.evaluate import EVAL_WORDS, W_EPISODES, W_RUN_LEN, W_RUN_SUM, W_STEPS, reduce_steps
from hftlob.layout import INFO_AGENT_WORDS, INFO_EXE, INFO_MM, INFO_WORLD, INFO_WORLD_WORDS
from hftlob.train import diag as D
from hftlob.train import ippo as I
from hftlob.train import population as POP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")
R, M = _lib.DIAG_STRIPE_ROWS, _lib.DIAG_MAX_STRIPES
NEW = ("hftlob_rollout_diag", "hftlob_rollout_diag_workspace", "hftlob_world_tally")


# ------------------------------------------------------------------ ABI
def _define(name: str) -> int:
    return int(re.search(rf"#define {name}\s+(\d+)", open(HEADER).read()).group(1))


def test_header_exports_and_constants():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(hftlob_[a-z_]+)\s*\(", src))
    for sym in NEW:
        assert sym in declared and sym in _lib.EXPORTS
    assert _define("HFTLOB_ABI_VERSION") == 8 == _lib.ABI_VERSION
    assert _define("HFTLOB_DIAG_WORDS") == _lib.DIAG_WORDS == D.DIAG_WORDS == 86
    assert _define("HFTLOB_WORLD_TALLY_WORDS") == _lib.WORLD_TALLY_WORDS == D.WORLD_TALLY_WORDS == 2 * INFO_WORLD_WORDS
    assert (_define("HFTLOB_DIAG_MAX_HEADS"), _define("HFTLOB_DIAG_MAX_ACTIONS")) == \
        (_lib.DIAG_MAX_HEADS, _lib.DIAG_MAX_ACTIONS) == (4, 16)
    assert (_define("HFTLOB_DIAG_STRIPE_ROWS"), _define("HFTLOB_DIAG_MAX_STRIPES")) == (R, M)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built")
    return _lib.lib()


def test_library_exports_the_new_symbols(L):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert all(s in syms for s in NEW)
    assert L.hftlob_version() == 8


def test_rollout_diag_argument_checks(L):
    """the documented codes, in the documented order, for pointers that are never dereferenced"""
    k = C.c_void_p(64)
    f = L.hftlob_rollout_diag
    nv = lambda *n: (C.c_int * len(n))(*n)  # noqa: E731
    ok = [k] * 7                                           # action, reward, value, log_prob, adv, target, done
    assert f(-1, 1, nv(3), *ok, k, k, None) == -3          # N < 0
    assert b"N" in L.hftlob_last_error()
    assert f(-1, 0, None, *([None] * 7), None, None, None) == -3   # ... before everything else
    for K in (0, 5, -1):
        assert f(8, K, nv(3, 3, 3, 3, 3), *ok, k, k, None) == -3   # K outside 1..4
    assert f(8, 0, None, *ok, k, k, None) == -3            # (the shape before the NULL nvec)
    assert f(8, 1, None, *ok, k, k, None) == -2            # NULL nvec
    assert f(8, 1, nv(3), *ok, None, k, None) == -2        # NULL diag
    assert f(0, 1, nv(3), *([None] * 7), None, None, None) == -2   # N = 0 still needs diag
    for j in range(7):                                     # each NULL array
        args = list(ok)
        args[j] = None
        assert f(8, 1, nv(3), *args, k, k, None) == -2, j
    assert f(8, 1, nv(3), *ok, k, None, None) == -2        # NULL workspace
    assert f(8, 1, nv(17), *ok, None, k, None) == -2       # (the NULL diag before the nvec entry)
    for bad in ((0,), (17,), (-1,), (3, 0), (16, 3, 16, 17)):
        assert f(8, len(bad), nv(*bad), *ok, k, k, None) == -1, bad   # an nvec entry outside 1..16
    assert b"nvec" in L.hftlob_last_error()


def test_world_tally_argument_checks(L):
    k = C.c_void_p(64)
    f = L.hftlob_world_tally
    assert f(0, 1, 86, k, 0, k, None) == -3
    assert f(4, 0, 86, k, 0, k, None) == -3
    assert f(4, 1, INFO_WORLD_WORDS - 1, k, 0, k, None) == -3
    assert f(0, 1, 86, None, 0, None, None) == -3          # the shape before the pointers
    assert f(4, 1, 86, None, 0, k, None) == -2
    assert f(4, 1, 86, k, 0, None, None) == -2
    assert f(4, 1, 86, k, 1 << INFO_WORLD_WORDS, k, None) == -1
    assert f(4, 1, 86, None, 1 << INFO_WORLD_WORDS, k, None) == -2   # the pointers before the mask


def _stripe_rule(N):
    rows = R if -(-N // R) <= M else -(-N // M)
    return rows, (-(-N // rows) if N > 0 else 0)


@pytest.mark.parametrize("N", [0, 1, R - 1, R, R + 1, M * R - 1, M * R, M * R + 1, 3 * M * R + 7, 2 ** 33 + 5])
def test_workspace_follows_the_stripe_rule(L, N):
    rows, G = _stripe_rule(N)
    assert G <= M and (N == 0 or (G - 1) * rows < N <= G * rows)      # no stripe is empty
    assert L.hftlob_rollout_diag_workspace(N) == G * 86 == D.diag_workspace(N)
    assert (D.stripe_rows(N), D.stripes(N)) == (rows, G)


def test_workspace_refuses_a_negative_size(L):
    assert L.hftlob_rollout_diag_workspace(-1) == -3


# ------------------------------------------------------------------ rollout_diag_reference
def diag_case(N, nvec, seed=0):
    """(action [N, K], reward, value, log_prob, done), adv, target: float columns that mix +-1e8 with values
    near 1e-3, action words that include -1 and nvec[k]"""
    g = torch.Generator().manual_seed(seed * 1000003 + N)
    K = len(nvec)
    action = torch.stack([torch.randint(-1, n + 1, (N,), generator=g, dtype=torch.int32) for n in nvec], 1)
    if N >= 2 * K:   # both out-of-range values in every head, whatever the draw
        for k, n in enumerate(nvec):
            action[2 * k, k], action[2 * k + 1, k] = -1, n

    def col():
        big = torch.rand(N, generator=g) < 0.1
        sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
        return torch.where(big, sign * 1e8 * (1.0 + torch.rand(N, generator=g)), 1e-3 * torch.randn(N, generator=g))

    reward, value, log_prob, adv, target = (col().float().contiguous() for _ in range(5))
    done = torch.rand(N, generator=g) < 0.2
    return (action.contiguous(), reward, value, log_prob, done), adv, target


DIAG_SIZES = [1, R - 1, R, R + 1, M * R + 1]
DIAG_HEADS = [[1], [16, 3, 16, 1]]


def _two_product(r):
    """the squares of float64 values exactly, as two float64 arrays hi + lo (Veltkamp's split, Dekker's product)"""
    hi = r * r
    c = 134217729.0 * r
    a = c - (c - r)
    b = r - a
    lo = ((a * a - hi) + 2.0 * a * b) + b * b
    return hi, lo


@pytest.mark.parametrize("nvec", DIAG_HEADS, ids=["K1", "K4"])
@pytest.mark.parametrize("N", DIAG_SIZES)
def test_rollout_diag_reference(N, nvec):
    buf, adv, target = diag_case(N, nvec)
    out = D.rollout_diag_reference(buf, adv, target, nvec)
    assert out.dtype == torch.float64 and tuple(out.shape) == (86,)
    got = out.tolist()
    action, reward, value, log_prob, done = (x.numpy() for x in buf)
    want = np.zeros(86)
    want[0], want[1] = N, int(done.sum())
    for k, n in enumerate(nvec):
        a = action[:, k].astype(np.int64)
        ok = (a >= 0) & (a < n)
        want[14 + k], want[18 + k] = a[ok].sum(), (~ok).sum()
        want[22 + 16 * k:22 + 16 * k + n] = np.bincount(a[ok], minlength=n)
        if N >= 8:
            assert want[18 + k] >= 2                       # -1 and nvec[k] are there
    exact = [0, 1] + list(range(14, 86))
    assert [got[w] for w in exact] == [want[w] for w in exact]
    v64, t64 = value.astype(np.float64), target.numpy().astype(np.float64)
    cols = [reward.astype(np.float64), v64, log_prob.astype(np.float64), adv.numpy().astype(np.float64), t64, t64 - v64]
    checked = set(exact)
    for q, x in enumerate(cols):
        s_abs, s_sq = math.fsum(np.abs(x).tolist()), None
        hi, lo = _two_product(x)
        if q < 5:
            assert not lo.any()                            # a widened float32 squares exactly
        s_sq = math.fsum(hi.tolist() + lo.tolist())
        assert abs(got[2 + 2 * q] - math.fsum(x.tolist())) <= N * 2.0 ** -52 * s_abs, (q, "sum")
        assert abs(got[3 + 2 * q] - s_sq) <= N * 2.0 ** -52 * s_sq, (q, "sum of squares")
        checked |= {2 + 2 * q, 3 + 2 * q}
    assert checked == set(range(86))                       # no word is left out


def test_rollout_diag_reference_follows_the_stated_order():
    """a case where the order shows: the lanes' interleave, then lane order, then stripe order, in plain Python"""
    N, nvec = R + 300, [3]
    buf, adv, target = diag_case(N, nvec, seed=5)
    out = D.rollout_diag_reference(buf, adv, target, nvec).tolist()
    x = buf[1].double().tolist()
    rows, G = _stripe_rule(N)
    tot = None
    for g in range(G):
        lanes = [0.0] * 256
        for i in range(g * rows, min(N, (g + 1) * rows)):
            lanes[(i - g * rows) % 256] += x[i]
        part = lanes[0]
        for l in range(1, 256):
            part += lanes[l]
        tot = part if tot is None else tot + part
    assert out[2] == tot


def test_rollout_diag_reference_of_nothing_is_zero():
    e = torch.empty(0)
    out = D.rollout_diag_reference((torch.empty((0, 2), dtype=torch.int32), e, e, e, torch.empty(0, dtype=torch.bool)),
                                   e, e, [3, 4])
    assert torch.equal(out, torch.zeros(86, dtype=torch.float64))


def test_rollout_diag_checks_its_arguments():
    buf, adv, target = diag_case(8, [3])
    for nvec in ([], [3] * 5, [17], [0]):
        with pytest.raises(ValueError, match="heads"):
            D.rollout_diag_reference(buf, adv, target, nvec)
    with pytest.raises(ValueError, match="action"):
        D.rollout_diag_reference(buf, adv, target, [3, 3])
    with pytest.raises(ValueError, match="adv"):
        D.rollout_diag_reference(buf, adv.double(), target, [3])
    with pytest.raises(ValueError, match="contiguous"):
        D.rollout_diag_reference(buf, torch.zeros(16)[::2], target, [3])
    with pytest.raises(ValueError, match="GPU"):
        D.rollout_diag(buf, adv, target, [3])              # the launch has no CPU path


# ------------------------------------------------------------------ world_tally_reference
def info_records(T, E, A, seed=0):
    """int32 [T, E, 14 + 24 A] info records: ints of both signs (some above 2^26) and float32 bits where the
    layout has floats"""
    g = torch.Generator().manual_seed(seed)
    W = INFO_WORLD_WORDS + A * INFO_AGENT_WORDS
    ints = torch.randint(-2 ** 28, 2 ** 28, (T, E, W), generator=g, dtype=torch.int32)
    fl = (torch.randn((T, E, W), generator=g) * 100.0).float().view(torch.int32)
    isf = [bool(f) for _, f in INFO_WORLD]
    for fields in [INFO_MM, INFO_EXE, INFO_EXE][:A]:       # LAYOUT's agents: the floats where reduce_steps reads floats
        isf += [bool(f) for _, f in fields] + [False] * (INFO_AGENT_WORDS - len(fields))
    return torch.where(torch.tensor(isf), fl, ints).contiguous()


def test_world_tally_reference_is_a_plain_double_loop():
    T, E = 5, 3
    info = info_records(T, E, 2)
    start = torch.rand((E, 28), dtype=torch.float64)
    keep = start.clone()
    got = D.world_tally_reference(info, start)
    assert torch.equal(start, keep)                        # not modified
    want = keep.tolist()
    raw = info.numpy()
    for e in range(E):
        for k, (_, isf) in enumerate(INFO_WORLD):
            for t in range(T):
                x = float(raw[t, e, k:k + 1].view(np.float32)[0]) if isf else float(raw[t, e, k])
                want[e][2 * k] += x
                want[e][2 * k + 1] += x * x
    assert got.tolist() == want
    # from zeros, and cut into two calls
    assert torch.equal(D.world_tally_reference(info[3:], D.world_tally_reference(info[:3])), D.world_tally_reference(info))
    with pytest.raises(ValueError, match="info_words"):
        D.world_tally_reference(info[0])
    with pytest.raises(ValueError, match="wstats"):
        D.world_tally_reference(info, torch.zeros((E, 27), dtype=torch.float64))
    with pytest.raises(ValueError, match="GPU"):
        D.world_tally(info)


# ------------------------------------------------------------------ TrainDiag
LAYOUT = types.SimpleNamespace(agent_kinds=[0, 1, 1], agent_types=[0, 1, 1],
                               info_words=INFO_WORLD_WORDS + 3 * INFO_AGENT_WORDS)
NAMES = ["MM", "EXE"]


def make_diag(words, stats=None, wstats=None, E=2):
    stats = torch.zeros((E, 3, EVAL_WORDS), dtype=torch.float64) if stats is None else stats
    wstats = torch.zeros((E, 28), dtype=torch.float64) if wstats is None else wstats
    return D.TrainDiag(stats, wstats, words, LAYOUT, [[3], [2, 3]], [False, True], NAMES)


def words_of(action, reward, value, adv, target, nvec, done=None):
    N = reward.numel()
    done = torch.zeros(N, dtype=torch.bool) if done is None else done
    return D.rollout_diag_reference((action, reward, value, torch.zeros(N), done), adv, target, nvec)


def test_train_diag_actions_moments_and_names():
    N = 12
    a0 = torch.tensor([0, 0, 0, 1, 1, 2, 0, 0, 0, 0, 1, 2], dtype=torch.int32)
    a1 = torch.tensor([[0, 2], [1, 1]] * 6, dtype=torch.int32)
    tgt = torch.arange(N, dtype=torch.float32)
    w0 = words_of(a0, torch.ones(N), tgt.clone(), torch.arange(N).float(), tgt, [3], done=tgt > 9)   # a perfect predictor
    w1 = words_of(a1, torch.zeros(N), torch.full((N,), 2.0), torch.zeros(N), tgt, [2, 3])            # a constant one
    d = make_diag([w0, w1])
    h0 = d.actions(0)
    assert len(h0) == 1 and h0[0]["shares"] == [100 * 7 / 12, 100 * 3 / 12, 100 * 2 / 12]
    assert sum(h0[0]["shares"]) == pytest.approx(100.0) and h0[0]["out_of_range"] == 0
    assert h0[0]["mean"] == pytest.approx(float(a0.float().mean()))
    h1 = d.actions(1)
    assert [h["mean"] for h in h1] == [0.5, 1.5] and [len(h["shares"]) for h in h1] == [2, 3]
    m0, m1 = d.moments(0), d.moments(1)
    assert m0["explained_variance"] == 1.0 and m0["dones"] == 2
    assert m1["explained_variance"] == pytest.approx(0.0)        # Var(target - c) = Var(target)
    assert m0["reward"] == {"mean": 1.0, "std": 0.0}
    assert m0["target"]["mean"] == 5.5 and m0["target"]["std"] == pytest.approx(float(tgt.double().std(unbiased=False)))
    assert set(m0) == {"reward", "value", "log_prob", "advantage", "target", "explained_variance", "dones"}
    # a constant target: no variance to explain
    wc = words_of(a0, torch.ones(N), tgt, torch.zeros(N), torch.full((N,), 3.0), [3])
    assert math.isnan(make_diag([wc, w1]).moments(0)["explained_variance"])
    # out of range: in no bin, not in the mean, and the shares fall short of 100
    a_bad = a0.clone()
    a_bad[0], a_bad[1] = -1, 3
    hb = make_diag([words_of(a_bad, torch.ones(N), tgt, tgt, tgt, [3]), w1]).actions(0)[0]
    assert hb["out_of_range"] == 2 and sum(hb["shares"]) == pytest.approx(100 * 10 / 12)
    assert hb["mean"] == pytest.approx(float(a_bad[2:].float().mean()))


def test_train_diag_of_nothing_is_nan():
    z = torch.zeros(86, dtype=torch.float64)
    d = make_diag([z, z])
    assert all(math.isnan(s) for s in d.actions(0)[0]["shares"]) and math.isnan(d.actions(1)[1]["mean"])
    m = d.moments(0)
    assert math.isnan(m["value"]["mean"]) and math.isnan(m["explained_variance"]) and m["dones"] == 0
    assert all(math.isnan(v["mean"]) and math.isnan(v["std"]) for v in d.world().values())
    s = d.summary()
    assert math.isnan(s["agent_MM/episode_reward_mean"]) and s["agent_MM/episodes"] == 0
    assert math.isnan(s["world/spread_mean"]) and math.isnan(s["agent_EXE/quant_left_mean"])


def test_train_diag_summary_keys_and_world():
    T, E = 4, 2
    info = info_records(T, E, 3, seed=3)
    rew = torch.rand((T, E, 3))
    done = torch.tensor([[False, False], [True, False], [False, False], [True, True]])
    stats = reduce_steps(rew, info, done, LAYOUT)
    wstats = D.world_tally_reference(info)
    N = T * E
    w0 = words_of(torch.zeros(N, dtype=torch.int32), rew[:, :, 0].reshape(-1).contiguous(), torch.zeros(N), torch.zeros(N),
                  torch.ones(N), [3])
    w1 = words_of(torch.ones((2 * N, 2), dtype=torch.int32), torch.zeros(2 * N), torch.zeros(2 * N), torch.zeros(2 * N),
                  torch.ones(2 * N), [2, 3])
    d = make_diag([w0, w1], stats, wstats)
    later = stats.clone()
    stats.zero_(), wstats.zero_(), w0.zero_()                  # the diag holds clones
    assert torch.equal(d.stats.stats, later)
    s = d.summary()
    want = set()
    for name, fields in (("MM", INFO_MM), ("EXE", INFO_EXE)):
        want |= {f"agent_{name}/{f}_{m}" for f, _ in fields for m in ("mean", "std")}
        want |= {f"agent_{name}/{k}" for k in ("episodes", "episode_reward_mean", "episode_length_mean",
                                               "explained_variance", "value_mean", "advantage_std")}
    want |= {"agent_MM/action_0", "agent_MM/action_1", "agent_MM/action_2",
             "agent_EXE/action_dim_0_mean_quant", "agent_EXE/action_dim_1_mean_quant"}
    want |= {f"world/{k}_mean" for k, _ in INFO_WORLD}
    assert set(s) == want
    assert s["agent_MM/action_0"] == 100.0 and s["agent_EXE/action_dim_1_mean_quant"] == 1.0
    assert s["agent_MM/episodes"] == 3 and s["agent_EXE/episodes"] == 6
    raw = info[:, :, :INFO_WORLD_WORDS]
    x = torch.where(torch.tensor([bool(f) for _, f in INFO_WORLD]), raw.view(torch.float32).double(), raw.double())
    w = d.world()
    assert list(w) == [k for k, _ in INFO_WORLD]
    for k, (name, _) in enumerate(INFO_WORLD):
        assert w[name]["mean"] == pytest.approx(float(x[:, :, k].mean()), rel=1e-12)
        assert w[name]["std"] == pytest.approx(float(x[:, :, k].std(unbiased=False)), rel=1e-9)
        assert s[f"world/{name}_mean"] == w[name]["mean"]
    k = [f for f, _ in INFO_MM].index("inventory")
    inv = info[:, :, INFO_WORLD_WORDS + k].double()
    assert s["agent_MM/inventory_mean"] == pytest.approx(float(inv.mean()), rel=1e-12)


# ------------------------------------------------------------------ the CPU trainer on a stand-in env
class _Space:
    def __init__(self, n=None, shape=None):
        self.n, self.shape = n, shape


class _MAC:
    number_of_agents_per_type = [1, 2]


class DiagEnv:
    """CPU stand-in with MARLEnv's interface (tests/test_ippo.py's FakeEnv with independent rows): an env's obs,
    rewards and info record are functions of its own key, step count and action words; episodes end every 5
    steps.  Type 0 is Discrete(3), type 1 MultiDiscrete([2, 3]) with two agents.  ``return_info="raw"``: the
    step fills ``last_rewards`` and ``last_info_words`` and returns {} for the info; every step is recorded."""
    device = torch.device("cpu")
    list_of_agents_configs = [object(), object()]
    multi_agent_config = _MAC()
    observation_spaces = [_Space(shape=(3,)), _Space(shape=(4,))]
    action_spaces = [_Space(n=3), _Space(n=[2, 3])]
    default_params = None
    layout = LAYOUT
    type_names = NAMES
    return_info = "raw"
    FLOATS = torch.tensor([bool(f) for _, f in INFO_WORLD]
                          + [bool(f) for _, f in INFO_MM] + [False] * (INFO_AGENT_WORDS - len(INFO_MM))
                          + ([bool(f) for _, f in INFO_EXE] + [False] * (INFO_AGENT_WORDS - len(INFO_EXE))) * 2)

    def __init__(self):
        self.steps = []            # (rewards [E, 3], info [E, 86], done [E]) of every step

    def split_keys(self, keys, n):
        k = keys.to(torch.int64)
        j = torch.arange(n, dtype=torch.int64)
        return ((k[:, None, :] * 1_000_003 + j[None, :, None] * 7919 + 17) % (2 ** 31)).to(torch.int32)

    @staticmethod
    def _obs(seed, n, d):
        i = torch.arange(n * d, dtype=torch.int64).view(1, n, d)
        return ((seed[:, None, None] * 2654435761 + i * 40503 + 12345) % 65536).float() / 32768.0 - 1.0

    def reset(self, keys, params):
        k = keys.to(torch.int64)
        seed = k[:, 0] * 31 + k[:, 1]
        return [self._obs(seed, 1, 3), self._obs(seed + 1, 2, 4)], torch.zeros(keys.shape[0], dtype=torch.int64)

    def step(self, keys, state, actions, params):
        E = keys.shape[0]
        assert actions[0].shape == (E, 1) and actions[1].shape == (E, 2, 2)
        k, t = keys.to(torch.int64), state + 1
        a = actions[0].view(E).to(torch.int64) + 3 * actions[1].reshape(E, -1).to(torch.int64).sum(-1)
        seed = k[:, 0] * 31 + k[:, 1] * 17 + t * 13 + a * 7
        done = t % 5 == 0
        r0 = (actions[0].view(E, 1) == 0).float() + (seed % 11)[:, None].float() / 11.0
        r1 = (seed % 7)[:, None].float().repeat(1, 2) / 7.0 - actions[1].float().sum(-1) * 0.25
        j = torch.arange(self.layout.info_words, dtype=torch.int64)[None]
        v = (seed[:, None] * 2654435761 + j * 40503) % 2001 - 1000                       # [E, 86] ints
        self.last_info_words = torch.where(self.FLOATS, (v.float() / 8.0).view(torch.int32), v.to(torch.int32))
        self.last_rewards = torch.cat([r0, r1], 1).contiguous()
        self.steps.append((self.last_rewards.clone(), self.last_info_words.clone(), done.clone()))
        dones = {"__all__": done, "agents": [done[:, None], done[:, None].repeat(1, 2)]}
        return [self._obs(seed, 1, 3), self._obs(seed + 1, 2, 4)], t, [r0, r1], dones, {}


def config(**kw):
    return I.default_config(**{**dict(NUM_ENVS=8, NUM_STEPS=10, GRU_HIDDEN_DIM=16, FC_DIM_SIZE=16, NUM_MINIBATCHES=2,
                                      UPDATE_EPOCHS=2, TOTAL_TIMESTEPS=8 * 10 * 10, CUDA_GRAPHS=False, SEED=3), **kw})


BASE_LOSS = ("total_loss", "value_loss", "actor_loss", "entropy", "approx_kl", "clip_frac")


def assert_same_training(a, b, la, lb):
    assert a.opt_count == b.opt_count and torch.equal(a.gen.get_state(), b.gen.get_state()) and torch.equal(a.rng, b.rng)
    for i in range(a.n_types):
        for (name, p), q in zip(a.nets[i].named_parameters(), b.nets[i].parameters()):
            assert torch.equal(p, q), (i, name)
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(torch.as_tensor(a.opts[i].state[p][key]), torch.as_tensor(b.opts[i].state[q][key]))
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(a.buf[i], f.name), getattr(b.buf[i], f.name)), (i, f.name)
    for ma, mb in zip(la, lb):
        for x, y in zip(ma["avg_reward"], mb["avg_reward"]):
            assert torch.equal(x, y)
        for x, y in zip(ma["loss"], mb["loss"]):
            for key in BASE_LOSS:
                assert torch.equal(x[key], y[key]), key


def expected_stats(steps, prev):
    """reduce_steps over an update's recorded steps, continued from words 2 and 3 of the update before"""
    rew, info, done = (torch.stack(x) for x in zip(*steps))
    carry = torch.zeros((rew.shape[1], 3, EVAL_WORDS), dtype=torch.float64)
    if prev is not None:
        carry[:, :, W_RUN_SUM], carry[:, :, W_RUN_LEN] = prev[:, :, W_RUN_SUM], prev[:, :, W_RUN_LEN]
    return reduce_steps(rew, info, done, LAYOUT, stats=carry), D.world_tally_reference(info)


def test_trainer_with_the_switch_trains_the_same_and_tallies_its_steps():
    updates, T = 3, 10
    env0 = DiagEnv()
    plain = I.IPPOTrainer(env0, config())
    lp = [plain.update() for _ in range(updates)]
    assert all(set(m) == {"loss", "avg_reward"} and set(m["loss"][0]) == set(BASE_LOSS) for m in lp)   # today's keys
    env = DiagEnv()
    tr = I.IPPOTrainer(env, config(TRAIN_DIAG=True))
    firsts, run = [], tr._run_step
    tr._run_step = lambda s: firsts.append((list(s["types"]), run(s))) or firsts[-1][1]
    ld, prev = [], None
    for u in range(updates):
        n0 = len(firsts)
        m = tr.update()
        ld.append(m)
        d = m["diag"]
        assert isinstance(d, D.TrainDiag)
        want, wwant = expected_stats(env.steps[u * T:(u + 1) * T], prev)
        assert torch.equal(d.stats.stats, want) and torch.equal(d.wstats, wwant)
        prev = want
        assert d.stats.steps(0) == 8 * T and d.stats.episodes(1) == 2 * 8 * 2      # two episode ends per update
        for i in range(2):
            ref = D.rollout_diag_reference(tr.buf[i], tr._st[i]["adv"], tr._st[i]["tgt"], tr.nets[i].heads)
            assert torch.equal(d.words[i], ref) and d.words[i][0] == T * tr.n_actors[i]
            first = next(r[t.index(i)] for t, r in firsts[n0:] if i in t)      # the type's first minibatch step
            assert torch.equal(m["loss"][i]["approx_kl_0"], first[4])
            assert torch.equal(m["loss"][i]["clip_frac_0"], first[5])
            assert set(m["loss"][i]) == set(BASE_LOSS) | {"approx_kl_0", "clip_frac_0"}
        assert float(m["loss"][0]["approx_kl_0"]) == pytest.approx(0.0, abs=1e-6)   # ratio_0: the same log-probs
        s = d.summary()
        assert s["agent_EXE/action_dim_0_mean_quant"] == pytest.approx(float(tr.buf[1].action[..., 0].float().mean()))
        assert sum(s[f"agent_MM/action_{a}"] for a in range(3)) == pytest.approx(100.0)
        assert s["agent_MM/episode_length_mean"] == 5.0
    assert_same_training(tr, plain, ld, lp)
    # an earlier update's diag was not overwritten by the later rollouts
    assert torch.equal(ld[0]["diag"].stats.stats, expected_stats(env.steps[:T], None)[0])
    for a, b in zip(env.steps, env0.steps):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_episodes_spanning_two_rollouts_count_whole():
    """NUM_STEPS = 4 against episodes of 5 steps: the running sum and length carry across the updates"""
    env = DiagEnv()
    tr = I.IPPOTrainer(env, config(TRAIN_DIAG=True, NUM_STEPS=4, TOTAL_TIMESTEPS=8 * 4 * 10))
    ms = [tr.update()["diag"] for _ in range(5)]
    rew, info, done = (torch.stack(x) for x in zip(*env.steps))
    whole = reduce_steps(rew, info, done, LAYOUT)
    assert sum(d.stats.episodes(0) for d in ms) == 8 * 4
    assert all(d.stats.episode_length(0)["mean"] == 5.0 for d in ms if d.stats.episodes(0))
    assert ms[0].stats.episodes(0) == 0 and ms[1].stats.episodes(0) == 8
    w_ep = 4   # W_EP_SUM: the completed episodes' reward sums, added whole
    assert sum(float(d.stats.stats[:, :, w_ep].sum()) for d in ms) == pytest.approx(float(whole[:, :, w_ep].sum()), rel=1e-12)
    assert int(whole[:, 0, W_EPISODES].sum()) == 8 * 4 and int(whole[:, 0, W_STEPS].sum()) == 8 * 20


def test_population_member_diag_equals_its_solo_run():
    members = [dict(SEED=3, LR=[3e-3, 1e-3]), dict(SEED=4, LR=[1e-3, 1e-3], GAMMA=[0.99, 0.9])]
    updates = 2
    solos = []
    for kw in members:
        tr = I.IPPOTrainer(DiagEnv(), config(TRAIN_DIAG=True, **kw))
        solos.append((tr, [tr.update() for _ in range(updates)]))
    pop = POP.PopulationTrainer(DiagEnv(), [config(TRAIN_DIAG=True, **kw) for kw in members])
    metrics = [pop.update() for _ in range(updates)]
    assert pop._tally.stats.shape[0] == 2 * 8 and all(m._tally is pop._tally for m in pop.members)
    for k, (solo, ls) in enumerate(solos):
        lm = [ms[k] for ms in metrics]
        assert_same_training(pop.members[k], solo, lm, ls)
        for a, b in zip(lm, ls):
            assert torch.equal(a["diag"].stats.stats, b["diag"].stats.stats)
            assert torch.equal(a["diag"].wstats, b["diag"].wstats)
            assert all(torch.equal(x, y) for x, y in zip(a["diag"].words, b["diag"].words))
            for i in range(2):
                assert torch.equal(a["loss"][i]["approx_kl_0"], b["loss"][i]["approx_kl_0"])
            assert {k_: v for k_, v in a["diag"].summary().items() if v == v} == \
                {k_: v for k_, v in b["diag"].summary().items() if v == v}
    assert not torch.equal(metrics[0][0]["diag"].stats.stats, metrics[0][1]["diag"].stats.stats)
    logged = []
    POP.train_population(DiagEnv(), [config(TRAIN_DIAG=True, **kw) for kw in members], 1, log=logged.append)
    assert len(logged) == 2 and all("agent_MM/action_0" in rec["diag"] for rec in logged)


def test_train_logs_the_summary_and_main_has_the_flag():
    logged = []
    I.train(DiagEnv(), config(TRAIN_DIAG=True), 2, log=logged.append)
    assert [r["update"] for r in logged] == [0, 1] and all("world/spread_mean" in r["diag"] for r in logged)
    logged = []
    I.train(DiagEnv(), config(), 1, log=logged.append)
    assert "diag" not in logged[0]
    sw = next(s for s in I.SWITCHES if s.key == "TRAIN_DIAG")
    assert sw.flag == "--train-diag" and sw.gpu is False and I.default_config()["TRAIN_DIAG"] is False


def test_the_switch_needs_an_env_that_writes_the_info_record():
    class NoInfo(DiagEnv):
        return_info = False

    with pytest.raises(ValueError, match='return_info="raw"'):
        I.IPPOTrainer(NoInfo(), config(TRAIN_DIAG=True))
    I.IPPOTrainer(NoInfo(), config())                           # without the switch any env will do

    class Wide(DiagEnv):
        action_spaces = [_Space(n=17), _Space(n=[2, 3])]

    with pytest.raises(ValueError, match=r"TRAIN_DIAG needs <= 16 actions.*agent type 0"):
        I.IPPOTrainer(Wide(), config(TRAIN_DIAG=True))
