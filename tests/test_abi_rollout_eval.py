"""hftlob_env_rollout_eval without a GPU: the symbol is declared and exported, HFTLOB_EVAL_WORDS is
the host's constant, and the call rejects bad arguments with the documented codes before any device
work (include/hftlob.h; test_abi_rollout_actions.py's style: dummy pointers that are never
dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.layout import StepOut, pack_env_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")
NAME = "hftlob_env_rollout_eval"
OK, EINVAL, ENULL, ESHAPE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    return _lib.lib()


def test_declared_and_in_exports():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src), "declared in include/hftlob.h"
    assert NAME in _lib.EXPORTS
    assert re.search(r"#define\s+HFTLOB_ABI_VERSION\s+8\b", src)


def test_eval_words_constant():
    src = open(HEADER).read()
    m = re.search(r"#define\s+HFTLOB_EVAL_WORDS\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.EVAL_WORDS == 106
    from hftlob import evaluate
    from hftlob.layout import INFO_AGENT_WORDS
    assert evaluate.EVAL_WORDS == 106 and 8 + 2 * (1 + INFO_AGENT_WORDS) + 2 * INFO_AGENT_WORDS == 106


def test_symbol_exported(L):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert L.hftlob_version() == _lib.ABI_VERSION == 8


def test_error_codes(L):
    """R(cfg, n_env, n_steps, keys, actions, actions_fixed, msgs, init, state, stats, out, stream)"""
    R = getattr(L, NAME)
    c, _ = pack_env_cfg(builtin_config("2_player_fq_fqc"), 10, 100_000, True)
    k = C.c_void_p(64)
    full = StepOut(k, k, k, k, None)
    cfg, out = C.byref(c), C.byref(full)
    assert R(None, 4, 8, k, k, 0, k, k, k, k, out, None) == ENULL              # null cfg: check_env first
    bad, _ = pack_env_cfg(builtin_config("2_player_fq_fqc"), 10, 100_000, True)
    bad.ep_type = 2                                                            # a config the env launches refuse
    assert R(C.byref(bad), 4, 8, k, k, 0, k, k, k, k, out, None) == EINVAL
    assert R(C.byref(bad), 0, 0, None, None, 1, None, None, None, None, None, None) == EINVAL  # before the sizes
    bad2, _ = pack_env_cfg(builtin_config("2_player_fq_fqc"), 10, 100_000, True)
    bad2.action_words += 1
    assert R(C.byref(bad2), 4, 8, k, k, 1, k, k, k, k, out, None) == EINVAL
    for fixed in (0, 1):
        assert R(cfg, 4, 0, k, k, fixed, k, k, k, k, out, None) == ESHAPE      # n_steps = 0: the last step always emits
        assert R(cfg, 0, 8, k, k, fixed, k, k, k, k, out, None) == ESHAPE      # n_env = 0
        assert R(cfg, 4, -1, k, k, fixed, k, k, k, k, out, None) == ESHAPE
        assert R(cfg, -1, 8, k, k, fixed, k, k, k, k, out, None) == ESHAPE
        assert R(cfg, 0, 8, None, None, fixed, None, None, None, None, None, None) == ESHAPE  # sizes before pointers
        for hole, what in enumerate(("keys", "actions", "msgs", "init", "state", "stats", "out")):
            args = [k, k, fixed, k, k, k, k, out]
            args[hole if hole < 2 else hole + 1] = None
            assert R(cfg, 4, 8, *args, None) == ENULL, what
            assert b"null" in L.hftlob_last_error()
    for field in ("obs", "rewards", "done_all", "dones"):                      # the required outputs (the last step's)
        o = StepOut(k, k, k, k, None)
        setattr(o, field, None)
        assert R(cfg, 4, 8, k, k, 0, k, k, k, k, C.byref(o), None) == ENULL, field
        assert b"null output" in L.hftlob_last_error()


def test_rollout_eval_argument_checks_need_no_device():
    """MARLEnv.rollout_eval's key checks raise before any device call"""
    import torch
    from hftlob.env import MARLEnv
    assert callable(MARLEnv.rollout_eval)
    with pytest.raises(ValueError, match=r"\[T, E, 2\]"):
        MARLEnv.rollout_eval(None, torch.zeros((4, 2), dtype=torch.int32), None, None, None)
    with pytest.raises(ValueError, match="T >= 1"):
        MARLEnv.rollout_eval(None, torch.zeros((0, 4, 2), dtype=torch.int32), None, None, None)
