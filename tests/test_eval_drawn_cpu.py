"""The drawn baseline without a GPU: the draw's definition (hftlob.evaluate.draw_actions_reference)
against a written-out loop over random_bits / gumbel_from_bits, its tie rule and distribution, the
Uniform policy entry and the checks that refuse an entry before any device work, the command line's
spelling, and the argument checks of hftlob_draw_actions / hftlob_env_rollout_eval_drawn (dummy
pointers that are never dereferenced, as in test_eval_mix_cpu.py)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.evaluate import Uniform, draw_actions_reference
from hftlob.layout import StepOut, pack_env_cfg
from hftlob.train.policy import gumbel_from_bits, random_bits

ALL13 = (1 << 13) - 1
# (n_actors, n_actions, allowed)
CASES = [(1, 2, 0b11), (5, 10, 0b1000010010), (7, 13, ALL13), (3, 32, (1 << 31) | 1)]
OK, EINVAL, ENULL, ESHAPE = 0, -1, -2, -3


def _key(k):
    return np.array([0, k], dtype=np.uint32)


@pytest.mark.parametrize("B,A,mask", CASES)
def test_definition_written_out(B, A, mask):
    """actor b takes the smallest allowed a that maximises the float32 Gumbel noise of the random word
    at counter (0, b A + a); the gap is the distance to the runner-up among the allowed"""
    for k in (0, 3, 0xDEADBEEF):
        acts, gaps = draw_actions_reference(_key(k), B, A, mask)
        assert acts.dtype == np.int32 and acts.shape == (B,) and gaps.shape == (B,)
        bits = random_bits(_key(k), B * A)
        for b in range(B):
            best, noises = -1, []
            for a in range(A):
                if not (mask >> a) & 1:
                    continue
                g = gumbel_from_bits(bits[b * A + a:b * A + a + 1])[0]
                if best < 0 or g > max(noises):
                    best = a
                noises.append(g)
            assert acts[b] == best, (k, b)
            assert (mask >> int(acts[b])) & 1, "only allowed actions appear"
            noises.sort()
            assert gaps[b] == np.float32(noises[-1] - noises[-2])


def test_one_bit_mask_draws_nothing():
    for k in range(5):
        acts, gaps = draw_actions_reference(_key(k), 9, 10, 1 << 7)
        assert (acts == 7).all() and np.isinf(gaps).all()
    acts, _ = draw_actions_reference(_key(1), 4, 32, 1 << 31)
    assert (acts == 31).all()


def test_exact_tie_takes_the_lower_action():
    row = np.array([[0.5, 2.0, -1.0, 2.0, 2.0, 9.0]], dtype=np.float32)
    acts, gaps = EV.masked_first_argmax(row, 0b011110)          # 9.0 is not allowed; 1, 3 and 4 tie
    assert acts.tolist() == [1] and gaps.tolist() == [0.0]
    acts, gaps = EV.masked_first_argmax(row, 0b011100)
    assert acts.tolist() == [3] and gaps.tolist() == [0.0]
    acts, gaps = EV.masked_first_argmax(row, 0b000101)
    assert acts.tolist() == [0] and gaps.tolist() == [1.5]
    with pytest.raises(ValueError):
        EV.masked_first_argmax(row, 0)
    with pytest.raises(ValueError):
        EV.masked_first_argmax(row, 1 << 6)


def test_distribution_is_uniform_over_the_set():
    """4096 actors, Uniform([1, 4, 7]) of 10: every count within 5 standard deviations of 4096 / 3
    (key (0, 1), chosen on the CPU: its largest deviation is 0.5 of one)"""
    n, mask = 4096, Uniform([1, 4, 7]).mask(10)
    acts, _ = draw_actions_reference(_key(1), n, 10, mask)
    counts = np.bincount(acts, minlength=10)
    assert counts.sum() == n and counts[[0, 2, 3, 5, 6, 8, 9]].sum() == 0
    sd = (n * (1 / 3) * (2 / 3)) ** 0.5
    assert (np.abs(counts[[1, 4, 7]] - n / 3) <= 5 * sd).all(), counts


def test_reference_refuses_bad_arguments():
    for args in ((0, 10, 1), (4, 0, 1), (4, 33, 1), (4, 10, 0), (4, 10, 1 << 10), (4, 10, -1)):
        with pytest.raises(ValueError):
            draw_actions_reference(_key(0), *args)


def test_uniform_entry():
    u = Uniform([1, 2, 3])
    assert u.actions == (1, 2, 3) and u == Uniform((1, 2, 3)) and hash(u) == hash(Uniform([1, 2, 3]))
    assert u.mask(10) == 0b1110 and Uniform([4]).mask(5) == 1 << 4
    assert Uniform.all().actions is None and Uniform.all().mask(13) == ALL13 and Uniform.all().mask(32) == 0xFFFFFFFF
    assert u.spelling() == "1+2+3" and Uniform.all().spelling() == "all"
    with pytest.raises(Exception):                                  # frozen
        u.actions = (1,)
    with pytest.raises(ValueError, match="empty"):
        Uniform([])
    with pytest.raises(ValueError, match="duplicate"):
        Uniform([1, 2, 1])
    with pytest.raises(ValueError, match="negative"):
        Uniform([1, -2])
    for bad in ([1.0], ["2"], [True], [None], "12", 3):
        with pytest.raises(TypeError, match="Uniform"):
            Uniform(bad)
    with pytest.raises(ValueError, match="outside"):
        u.mask(3)


def test_policy_entries_pass_a_uniform_through_and_lists_still_raise():
    net, u = torch.nn.Linear(1, 1), Uniform([0, 2])
    assert EV.policy_entries([net, u], 2) == [net, u]
    assert EV.policy_entries([Uniform.all(), [3]], 2) == [Uniform.all(), 3]
    with pytest.raises(NotImplementedError, match="Uniform"):
        EV.policy_entries([net, [1, 2]], 2)
    with pytest.raises(NotImplementedError, match="2 fixed actions"):
        EV.policy_entries([[1, 2], u], 2)
    assert EV.mix_entries("LB", [net, net], [4, u]) == [net, u]


def test_command_line_spelling():
    assert EV.parse_entries("1+2+3,all") == [Uniform([1, 2, 3]), Uniform.all()]
    assert EV.parse_entries("4,2") == [4, 2] and EV.parse_entries(" 4 , 0+1 ") == [4, Uniform([0, 1])]
    assert [EV.entry_spelling(p) for p in EV.parse_entries("4,0+1,all")] == [4, "0+1", "all"]
    with pytest.raises(ValueError):
        EV.parse_entries("1+x")
    with pytest.raises(ValueError):
        EV.parse_entries("1+1")
    ap = EV.build_parser()
    a = ap.parse_args(["--env-config", "c", "--uniform-actions", "1+2+3,all", "--envs", "4", "--steps", "5"])
    assert a.uniform_actions == "1+2+3,all" and a.fixed_actions is None and a.checkpoint is None
    for other in (["--fixed-actions", "4,2"], ["--checkpoint", "p"]):
        with pytest.raises(SystemExit):                             # one of the three
            ap.parse_args(["--env-config", "c", "--uniform-actions", "all,all", *other, "--envs", "4", "--steps", "5"])
    a = ap.parse_args(["--env-config", "c", "--checkpoint", "p", "--baseline-actions", "all,2", "--mix", "LB",
                       "--envs", "4", "--steps", "5"])
    assert EV.parse_entries(a.baseline_actions) == [Uniform.all(), 2]


class _HostOnly:
    """an env that holds what the entry checks read on the host and fails the test on anything else"""
    return_info = True

    def __init__(self, widths, sizes, partitionable=True):
        self.multi_agent_config = types.SimpleNamespace(number_of_agents_per_type=[1] * len(widths))
        self.action_widths = widths
        self.action_spaces = [types.SimpleNamespace(n=n) for n in sizes]
        self.cfg_c = types.SimpleNamespace(prng_partitionable=int(partitionable))

    def __getattr__(self, name):
        raise AssertionError(f"the entries must be checked before the env's {name} is touched")


@pytest.mark.parametrize("env_args,entries,text", [
    (([1, 3], [10, [11, 11, 11]]), [2, Uniform.all()], "MultiDiscrete"),
    (([1, 1], [10, 33]), [2, Uniform([1, 2])], "at most 32"),
    (([1, 1], [10, 13]), [Uniform([3, 10]), 2], "outside"),
    (([1, 1], [10, 13], False), [Uniform([3, 4]), 2], "prng_partitionable"),
], ids=["multidiscrete", "33_actions", "action_outside", "legacy_keys"])
def test_drawn_types_are_refused_before_any_device_work(env_args, entries, text):
    env = _HostOnly(*env_args)
    with pytest.raises(ValueError, match=text):
        EV.evaluate_policy(env, entries, 4, 4, 0)
    with pytest.raises(ValueError, match=text):
        EV.evaluate_baseline(env, entries, 4, 4, 0)
    with pytest.raises(ValueError, match=text):
        EV.evaluate_combinations(env, [torch.nn.Linear(1, 1)] * 2, entries, 4, 4, 0)


def test_evaluate_baseline_checks_its_entries_first():
    env = _HostOnly([1, 1], [10, 13])
    with pytest.raises(NotImplementedError, match="Uniform"):
        EV.evaluate_baseline(env, [[1, 2], 2], 4, 4, 0)
    with pytest.raises(TypeError, match="evaluate_policy"):
        EV.evaluate_baseline(env, [torch.nn.Linear(1, 1), 2], 4, 4, 0)
    with pytest.raises(ValueError, match="outside"):
        EV.evaluate_baseline(env, [10, 2], 4, 4, 0)                 # a fixed action is a mask of one bit here
    with pytest.raises(ValueError, match="MultiDiscrete"):
        EV.evaluate_baseline(_HostOnly([1, 3], [10, [11] * 3]), [2, 2], 4, 4, 0)
    assert EV.draw_masks(env, [Uniform([1, 4]), 3]) == [0b10010, None]
    assert EV.draw_masks(env, [Uniform([1, 4]), 3], fixed_too=True) == [0b10010, 1 << 3]


def test_draw_actions_needs_a_gpu_key():
    with pytest.raises(ValueError, match="GPU"):
        EV.draw_actions(torch.zeros(2, dtype=torch.int32), 4, 10, 0b11)
    with pytest.raises(ValueError, match="key"):
        EV.draw_actions(torch.zeros(3, dtype=torch.int32), 4, 10, 0b11)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    return _lib.lib()


def test_draw_actions_error_codes(L):
    """R(n_actors, n_actions, allowed, key, actions, stream)"""
    assert "hftlob_draw_actions" in _lib.EXPORTS and "hftlob_env_rollout_eval_drawn" in _lib.EXPORTS
    R, k = L.hftlob_draw_actions, C.c_void_p(64)
    for args, text in (((0, 10, 1), b"n_actors"), ((-3, 10, 1), b"n_actors"), ((4, 0, 1), b"1..32"),
                       ((4, 33, 1), b"1..32"), ((4, 10, 0), b"empty"), ((4, 10, 1 << 10), b">= n_actions"),
                       ((4, 31, 1 << 31), b">= n_actions"), ((2 ** 31 - 1, 3, 1), b"counter")):
        assert R(*args, k, k, None) == EINVAL, args
        assert text in L.hftlob_last_error(), (args, L.hftlob_last_error())
    assert R(4, 10, 3, None, k, None) == EINVAL and b"null" in L.hftlob_last_error()
    assert R(4, 10, 3, k, None, None) == EINVAL and b"null" in L.hftlob_last_error()


def _cfg(name="2_player_fq_fqc", part=True, **exe):
    import dataclasses
    cfg = builtin_config(name)
    if exe:
        agents = dict(cfg.dict_of_agents_configs)
        agents["Execution"] = dataclasses.replace(agents["Execution"], **exe)
        cfg = dataclasses.replace(cfg, dict_of_agents_configs=agents)
    return pack_env_cfg(cfg, 10, 100_000, part)[0]


def test_rollout_eval_drawn_error_codes(L):
    """R(cfg, n_env, n_steps, keys, draw_keys, allowed, actions_out, msgs, init, state, stats, out, stream)"""
    R, k = L.hftlob_env_rollout_eval_drawn, C.c_void_p(64)
    out = StepOut(64, 64, 64, 64, None)
    c = _cfg()
    na = [int(c.types[t].n_actions) for t in range(2)]
    ok = (C.c_uint32 * 2)(1, (1 << na[1]) - 1)

    def call(cfg=c, n_env=4, n_steps=3, allowed=ok, **holes):
        a = dict(keys=k, draw_keys=k, actions_out=None, msgs=k, init=k, state=k, stats=k)
        a.update(holes)
        return R(C.byref(cfg), n_env, n_steps, a["keys"], a["draw_keys"], allowed, a["actions_out"], a["msgs"],
                 a["init"], a["state"], a["stats"], C.byref(out), None)

    assert call(n_env=0) == ESHAPE and call(n_steps=0) == ESHAPE
    for hole in ("keys", "draw_keys", "msgs", "init", "state", "stats"):
        assert call(**{hole: None}) == ENULL, hole
    assert call(allowed=None) == ENULL
    assert call(allowed=(C.c_uint32 * 2)(0, 1)) == EINVAL and b"empty" in L.hftlob_last_error()
    assert call(allowed=(C.c_uint32 * 2)(1, 1 << na[1])) == EINVAL and b">= n_actions" in L.hftlob_last_error()
    assert call(cfg=_cfg(part=False)) == EINVAL and b"prng_partitionable" in L.hftlob_last_error()
    md = _cfg(action_space="fixed_prices", n_actions=3, fixed_quant_value=11)
    assert call(cfg=md) == EINVAL and b"action_width" in L.hftlob_last_error()
    big = _cfg()
    big.types[1].n_actions = 33
    assert call(cfg=big, allowed=(C.c_uint32 * 2)(1, 1)) == EINVAL and b"1..32" in L.hftlob_last_error()
    assert na[1] >= 3                                               # so that 2^31 envs pass the 32-bit counter
    assert call(n_env=2 ** 31 - 1, allowed=ok) == EINVAL and b"counter" in L.hftlob_last_error()
