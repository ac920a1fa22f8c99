"""hftlob_eval_tally (hftlob.evaluate.tally_steps) against its definition, evaluate.reduce_steps, bit for
bit on synthetic step outputs.  The layout is that of the shipped 3_player_fq_fqc_dir config (A = 3,
MM and EXE kinds); T = 7; E = 5 and E = 70, whose E * A * 25 lanes (375, 5250) are no multiple of 64
and, at 70, span several 256-lane workgroups.  The reference is computed once per E and shared."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.layout import INFO_AGENT_WORDS, INFO_WORLD_WORDS, pack_env_cfg

pytestmark = pytest.mark.gpu

T = 7
EINVAL = -1
FLOATS = [0.1, 1e-3, 3e7, -0.1, -1e-3, -3e7, 12345.678, -0.33333334, 1.0, 0.0, 7.5e-5, -2.5e4]
INTS = [2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 27 + 1, -(2 ** 27 + 1), 0, 1, -1, 65, 100_000, -2_000_000, 2 ** 26 + 3, -(2 ** 31)]


@pytest.fixture(scope="module")
def layout():
    return pack_env_cfg(builtin_config("3_player_fq_fqc_dir"), 10, 100_000, True)[1]


def _inputs(layout, E, seed, isf=None):
    """Step outputs on the CPU: rewards float32 [T, E, A], info int32 [T, E, info_words], done bool [T, E].
    Every word cycles through its pool (FLOATS as bit patterns where ``isf`` marks a float word, else
    INTS) from a seeded offset, so every pool value appears in every agent's block; the world words hold
    noise the tally must not read."""
    A = len(layout.agent_kinds)
    isf = EV._float_words(layout).numpy() if isf is None else isf
    rng = np.random.default_rng(seed)
    fbits = np.array(FLOATS, np.float32).view(np.int32)
    ints = np.array(INTS, np.int64).astype(np.int32)
    info = rng.integers(-2 ** 31, 2 ** 31, (T, E, layout.info_words), dtype=np.int64).astype(np.int32)
    pick = rng.integers(0, len(FLOATS), (T, E, A, INFO_AGENT_WORDS))
    pick[:, :min(E, 4)] = (np.arange(T)[:, None, None, None] + np.arange(min(E, 4))[None, :, None, None] * 3
                           + np.arange(A)[None, None, :, None] + np.arange(INFO_AGENT_WORDS)[None, None, None, :]) % len(FLOATS)
    block = np.where(isf[None, None], fbits[pick], ints[pick])
    info[:, :, INFO_WORLD_WORDS:INFO_WORLD_WORDS + A * INFO_AGENT_WORDS] = block.reshape(T, E, -1)
    rew = np.array(FLOATS, np.float32)[rng.integers(0, len(FLOATS), (T, E, A))]
    # (a row picked with exact arithmetic so that, on the done patterns of envs 1 and 3 below, the plain
    # and the fused sum of the episode sums' squares round differently: checked in the first test)
    rew[:, :min(E, 4), 0] = np.array([-0.33333334, 3e7, 1e-3, -0.1, 7.5e-5, 0.1, 0.1], np.float32)[:, None]
    done = rng.random((T, E)) < 0.3
    done[:, 0] = False                                   # never
    done[:, 1] = False
    done[[0, T - 1], 1] = True                           # the first and the last step
    done[:, 2] = False
    done[[2, 3], 2] = True                               # two consecutive steps
    done[:, 3] = False
    done[[0, 3, 4, T - 1], 3] = True                     # all of them
    return torch.from_numpy(rew), torch.from_numpy(info), torch.from_numpy(done)


@pytest.fixture(scope="module", params=[5, 70], ids=["E5", "E70"])
def case(request, layout):
    """(E, device inputs, stats0, reduce_steps from zeros, reduce_steps from stats0): computed once"""
    E = request.param
    rew, info, done = (x.cuda() for x in _inputs(layout, E, seed=E))
    other = [x.cuda() for x in _inputs(layout, E, seed=1000 + E)]
    stats0 = EV.reduce_steps(*other, layout)             # a non-zero start, running sums included
    return {"E": E, "rew": rew, "info": info, "done": done, "stats0": stats0,
            "ref": EV.reduce_steps(rew, info, done, layout),
            "ref_from": EV.reduce_steps(rew, info, done, layout, stats0)}


def test_the_inputs_hold_the_inexact_cases(layout):
    """what makes a contracted multiply-add visible is in the data: int words whose squares are inexact
    in double, and a running reward sum whose square is"""
    for v in (2 ** 31 - 1, 2 ** 27 + 1):
        assert Fraction(float(v)) ** 2 != Fraction(float(v) * float(v))
    rew, info, done = _inputs(layout, 5, seed=5)
    assert not done[:, 0].any()
    # envs 1 and 3 end a later episode on a running sum whose square is inexact, and there the word "sum
    # of squares of the episodes' reward sums" differs between the plain sum and a fused multiply-add
    # (an episode's first end adds to 0, where the two agree, and env 2's second end follows its first
    # at once, on a single float)
    for e in (1, 3):
        run, plain, fused, inexact = 0.0, 0.0, 0.0, 0
        for t in range(T):
            run += float(rew[t, e, 0])
            if done[t, e]:
                inexact += Fraction(run) ** 2 != Fraction(run * run)
                plain = plain + run * run
                fused = float(Fraction(fused) + Fraction(run) ** 2)     # one rounding, as an FMA has
                run = 0.0
        assert inexact >= 1 and plain != fused, e
    isf = EV._float_words(layout).numpy()
    A = len(layout.agent_kinds)
    blk = info[:, :, INFO_WORLD_WORDS:].reshape(T, 5, A, INFO_AGENT_WORDS).numpy()
    for a in range(A):
        got_i = set(blk[:, :, a][:, :, ~isf[a]].reshape(-1).tolist())
        assert {2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 27 + 1} <= got_i
        if isf[a].any():
            got_f = set(blk[:, :, a][:, :, isf[a]].reshape(-1).view(np.float32).tolist())
            assert {np.float32(x).item() for x in (0.1, 1e-3, 3e7, -0.1, -3e7)} <= got_f
    assert isf.any() and not isf.all()


def test_bit_for_bit(case, layout):
    got = EV.tally_steps(case["rew"], case["info"], case["done"], layout)
    ref = case["ref"]
    assert got.dtype == torch.float64 and got.shape == ref.shape == (case["E"], 3, EV.EVAL_WORDS)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} words differ"
    # the reference is not trivial: steps, episodes per env, and sums that left the exact range
    assert bool((ref[:, :, EV.W_STEPS] == T).all())
    assert torch.equal(ref[:, 0, EV.W_EPISODES], case["done"].sum(0).double())
    assert float(ref[:, :, EV.W_STEP_Q + 1::2].max()) > 2.0 ** 61
    # the per-type rewards list of a per_step rollout is accepted as reduce_steps accepts it
    parts = [case["rew"][:, :, :1], case["rew"][:, :, 1:]]
    assert torch.equal(EV.tally_steps(parts, case["info"].reshape(T * case["E"], -1), case["done"], layout), ref)
    assert torch.equal(EV.tally_steps(case["rew"], case["info"], case["done"].view(torch.uint8), layout), ref)


@pytest.mark.parametrize("cuts", [(0, 3, 7), tuple(range(8))], ids=["3+4", "7x1"])
def test_continuation(case, layout, cuts):
    """from a non-zero start, the steps in several calls give the bits of one call, in place"""
    stats = case["stats0"].clone()
    for t0, t1 in zip(cuts, cuts[1:]):
        out = EV.tally_steps(case["rew"][t0:t1], case["info"][t0:t1], case["done"][t0:t1], layout, stats)
        assert out is stats
    assert torch.equal(stats, case["ref_from"])
    assert not torch.equal(case["ref_from"], case["ref"])
    one = EV.tally_steps(case["rew"], case["info"], case["done"], layout, case["stats0"].clone())
    assert torch.equal(one, case["ref_from"])


def test_partial_float_masks(layout, monkeypatch):
    """a mask that marks only some of an agent's words as float: the others are widened as int32, the
    bit pattern of 0.1f among them"""
    A, E = len(layout.agent_kinds), 5
    isf = np.zeros((A, INFO_AGENT_WORDS), bool)
    isf[0, [0, 5]] = True
    isf[1, 1::2] = True
    isf[2, [INFO_AGENT_WORDS - 1]] = True
    monkeypatch.setattr(EV, "_float_words", lambda lay: torch.from_numpy(isf))
    rew, info, done = _inputs(layout, E, seed=77, isf=isf)
    bits = int(np.array([0.1], np.float32).view(np.int32)[0])
    info[:, :, INFO_WORLD_WORDS + 1] = bits              # agent 0's word 1, an int word under this mask
    info[:, :, INFO_WORLD_WORDS + 5] = bits              # agent 0's word 5, a float word
    rew, info, done = rew.cuda(), info.cuda(), done.cuda()
    got = EV.tally_steps(rew, info, done, layout)
    assert torch.equal(got, EV.reduce_steps(rew, info, done, layout))
    assert bool((got[:, 0, EV.W_STEP_Q + 2 * (1 + 1)] == T * float(bits)).all())
    want = 0.0
    for _ in range(T):
        want += float(np.float32(0.1))
    assert bool((got[:, 0, EV.W_STEP_Q + 2 * (1 + 5)] == want).all())


def test_refused_arguments(case, layout):
    rew, info, done, E = case["rew"], case["info"], case["done"], case["E"]
    stats = torch.zeros((E, 3, EV.EVAL_WORDS), dtype=torch.float64, device="cuda")
    bad = [(rew.double(), info, done, None), (rew[:, :, :2], info, done, None), (rew[0], info, done, None),
           (rew, info.long(), done, None), (rew, info[:, :, :-1], done, None), (rew, info, done[:, 1:], None),
           (rew, info, done.float(), None), (rew[:0], info[:0], done[:0], None),          # n_steps = 0
           (rew.cpu(), info.cpu(), done.cpu(), None), (rew, info.cpu(), done, None), (rew, info, done.cpu(), None),
           (rew, info, done, stats.float()), (rew, info, done, stats[:, :2]), (rew, info, done, stats.cpu()),
           (rew, info, done, torch.zeros((E, 3, 2 * EV.EVAL_WORDS), dtype=torch.float64, device="cuda")[:, :, ::2])]
    for k, (r, i, d, s) in enumerate(bad):
        with pytest.raises(ValueError):
            EV.tally_steps(r, i, d, layout, s)
            pytest.fail(f"case {k} was accepted")
    assert not stats.any()                                # nothing was launched on the way


def test_abi_refuses_its_own_cases(case, layout):
    """hftlob_eval_tally with real device pointers: HFTLOB_EINVAL, and stats stay as they were"""
    L = _lib.lib()
    rew, info, done, E = case["rew"], case["info"], case["done"].view(torch.uint8), case["E"]
    stats = torch.zeros((E, 3, EV.EVAL_WORDS), dtype=torch.float64, device="cuda")
    fw = EV._float_word_masks(layout)
    p = [_lib.ptr(rew), _lib.ptr(info), _lib.ptr(done), fw, _lib.ptr(stats)]
    s = _lib.stream_ptr()
    iw = layout.info_words
    assert iw == INFO_WORLD_WORDS + 3 * INFO_AGENT_WORDS
    for n_env, n_agents, n_steps, words in ((0, 3, T, iw), (E, 0, T, iw), (E, 3, 0, iw), (E, 3, -1, iw),
                                            (E, 3, T, iw - 1), (E, 33, T, INFO_WORLD_WORDS + 33 * INFO_AGENT_WORDS)):
        assert L.hftlob_eval_tally(n_env, n_agents, n_steps, words, *p, s) == EINVAL
    for hole in range(5):
        q = list(p)
        q[hole] = None
        assert L.hftlob_eval_tally(E, 3, T, iw, *q, s) == EINVAL
    torch.cuda.synchronize()
    assert not stats.any()
    assert L.hftlob_eval_tally(E, 3, T, iw, *p, s) == 0   # and the same pointers with good sizes run
    assert torch.equal(stats, case["ref"])
