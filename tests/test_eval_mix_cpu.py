"""Mixed learned / baseline evaluation and the tally operator without a GPU: the combination names,
the policy-list checks (which raise before any device work), tally_steps' refusal of host tensors,
and hftlob_eval_tally's export and argument checks (include/hftlob.h; dummy pointers that are never
dereferenced, as in test_abi_rollout_eval.py)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.layout import INFO_AGENT_WORDS, INFO_WORLD_WORDS, pack_env_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")
NAME = "hftlob_eval_tally"
OK, EINVAL = 0, -1


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    return _lib.lib()


def test_combination_names():
    """the reference's order and naming: binary counting, 'L' for 1 and 'B' for 0, one character per type"""
    assert EV.combination_names(1) == ["B", "L"]
    assert EV.combination_names(2) == ["BB", "BL", "LB", "LL"]
    assert EV.combination_names(3) == ["BBB", "BBL", "BLB", "BLL", "LBB", "LBL", "LLB", "LLL"]
    with pytest.raises(ValueError):
        EV.combination_names(0)


def test_mix_entries():
    nets = [torch.nn.Linear(1, 1), torch.nn.Linear(1, 1)]
    assert EV.mix_entries("LB", nets, [4, [2]]) == [nets[0], [2]]
    assert EV.mix_entries("BL", nets, [4, 2]) == [4, nets[1]]
    for bad in ("L", "LBL", "LX", "lb"):
        with pytest.raises(ValueError, match="'L' or 'B'"):
            EV.mix_entries(bad, nets, [4, 2])


def test_policy_entries():
    net = torch.nn.Linear(1, 1)
    assert EV.policy_entries([net, 3], 2) == [net, 3]
    assert EV.policy_entries([[4], (2,)], 2) == [4, 2]
    with pytest.raises(ValueError, match="one network or fixed action per agent type"):
        EV.policy_entries([net], 2)
    with pytest.raises(NotImplementedError, match="2 fixed actions"):
        EV.policy_entries([net, [1, 2]], 2)
    for bad in ("4", 1.5, None, True, [2.0]):
        with pytest.raises(TypeError, match="agent type 1"):
            EV.policy_entries([net, bad], 2)


class _NoDevice:
    """an env that fails the test on any use beyond what the argument checks read"""
    return_info = True
    multi_agent_config = types.SimpleNamespace(number_of_agents_per_type=[1, 1])

    def __getattr__(self, name):
        raise AssertionError(f"the policy list must be checked before the env's {name} is touched")


@pytest.mark.parametrize("nets,exc", [([3], ValueError), ([3, 4, 5], ValueError), ([3, [1, 2]], NotImplementedError),
                                      ([3, "2"], TypeError), ([1.0, 2], TypeError)])
def test_policy_list_is_checked_before_any_device_work(nets, exc):
    with pytest.raises(exc):
        EV.evaluate_policy(_NoDevice(), nets, 4, 4, 0)
    with pytest.raises(exc):   # the same entries as the baseline side of the combinations
        EV.evaluate_combinations(_NoDevice(), [torch.nn.Linear(1, 1)] * 2, nets, 4, 4, 0)


def _layout():
    return pack_env_cfg(builtin_config("3_player_fq_fqc_dir"), 10, 100_000, True)[1]


def test_tally_steps_refuses_cpu_tensors():
    lay = _layout()
    T, E, A = 2, 3, len(lay.agent_kinds)
    rew = torch.zeros((T, E, A), dtype=torch.float32)
    info = torch.zeros((T, E, lay.info_words), dtype=torch.int32)
    done = torch.zeros((T, E), dtype=torch.bool)
    EV.reduce_steps(rew, info, done, lay)                     # the definition runs anywhere
    with pytest.raises(ValueError, match="GPU"):
        EV.tally_steps(rew, info, done, lay)


def test_tally_steps_checks_shapes_and_dtypes_on_the_host():
    lay = _layout()
    T, E, A = 2, 3, len(lay.agent_kinds)
    rew = torch.zeros((T, E, A), dtype=torch.float32)
    info = torch.zeros((T, E, lay.info_words), dtype=torch.int32)
    done = torch.zeros((T, E), dtype=torch.bool)
    with pytest.raises(ValueError, match="rewards"):
        EV.tally_steps(rew.double(), info, done, lay)
    with pytest.raises(ValueError, match="rewards"):
        EV.tally_steps(rew[:, :, :A - 1], info, done, lay)
    with pytest.raises(ValueError, match="at least one step"):
        EV.tally_steps(rew[:0], info[:0], done[:0], lay)
    with pytest.raises(ValueError, match="info_words"):
        EV.tally_steps(rew, info.long(), done, lay)
    with pytest.raises(ValueError, match="info_words"):
        EV.tally_steps(rew, info[:, :, :-1], done, lay)
    with pytest.raises(ValueError, match="done_all"):
        EV.tally_steps(rew, info, done[:, :E - 1], lay)
    with pytest.raises(ValueError, match="done_all"):
        EV.tally_steps(rew, info, done.float(), lay)


def test_float_word_masks():
    """bit k of an agent's mask is word k of _float_words' row"""
    lay = _layout()
    rows = EV._float_words(lay)
    masks = list(EV._float_word_masks(lay))
    assert len(masks) == len(lay.agent_kinds)
    for m, row in zip(masks, rows.tolist()):
        assert [bool((m >> k) & 1) for k in range(INFO_AGENT_WORDS)] == row
    assert len(set(masks)) > 1   # the MM and EXE kinds differ


def test_declared_and_exported(L):
    src = open(HEADER).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src), "declared in include/hftlob.h"
    assert NAME in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_error_codes(L):
    """R(n_env, n_agents, n_steps, info_words, rewards, info, done_all, float_words, stats, stream)"""
    R = getattr(L, NAME)
    k = C.c_void_p(64)
    fw = (C.c_uint32 * 32)()
    need = INFO_WORLD_WORDS + 3 * INFO_AGENT_WORDS
    for n_env, n_agents, n_steps in ((0, 3, 7), (-1, 3, 7), (5, 0, 7), (5, -2, 7), (5, 3, 0), (5, 3, -1)):
        assert R(n_env, n_agents, n_steps, need, k, k, k, fw, k, None) == EINVAL
        assert b">= 1" in L.hftlob_last_error()
    assert R(5, 3, 7, need - 1, k, k, k, fw, k, None) == EINVAL       # the third agent's block does not fit
    assert b"info_words" in L.hftlob_last_error()
    assert R(5, 33, 7, INFO_WORLD_WORDS + 33 * INFO_AGENT_WORDS, k, k, k, fw, k, None) == EINVAL   # > HFTLOB_MAX_AGENTS
    assert b"agents" in L.hftlob_last_error()
    for hole in range(5):
        args = [k, k, k, fw, k]
        args[hole] = None
        assert R(5, 3, 7, need, *args, None) == EINVAL, hole
        assert b"null" in L.hftlob_last_error()
