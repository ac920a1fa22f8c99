"""hftlob_env_rollout_actions without a GPU: the symbol is exported and the call rejects bad
arguments with the documented codes, in the documented order, before any device work
(include/hftlob.h; test_abi.py::test_error_null_and_shape's style: dummy pointers that are never
dereferenced)."""
import ctypes as C
import os
import subprocess

import pytest

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.layout import StepOut, pack_env_cfg

NAME = "hftlob_env_rollout_actions"
OK, EINVAL, ENULL, ESHAPE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    return _lib.lib()


def test_symbol_exported(L):
    assert NAME in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert L.hftlob_version() == _lib.ABI_VERSION == 8


def test_error_codes(L):
    """R(cfg, n_env, n_steps, keys, actions, msgs, init, state, out, per_step, stream)"""
    R = getattr(L, NAME)
    c, _ = pack_env_cfg(builtin_config("2_player_fq_fqc"), 10, 100_000, True)
    k = C.c_void_p(64)
    full = StepOut(k, k, k, k, None)
    cfg, out = C.byref(c), C.byref(full)
    assert R(None, 4, 8, k, k, k, k, k, out, 0, None) == ENULL              # null cfg: check_env first
    assert R(None, -1, -1, None, None, None, None, None, None, 0, None) == ENULL
    bad, _ = pack_env_cfg(builtin_config("2_player_fq_fqc"), 10, 100_000, True)
    bad.ep_type = 2
    assert R(C.byref(bad), -1, 8, k, k, k, k, k, out, 0, None) == EINVAL     # an invalid cfg before the sizes
    assert R(cfg, -1, 8, k, k, k, k, k, out, 0, None) == ESHAPE             # negative n_env
    assert R(cfg, 4, -1, k, k, k, k, k, out, 0, None) == ESHAPE             # negative n_steps
    assert R(cfg, -1, 0, None, None, None, None, None, None, 0, None) == ESHAPE  # sizes before the empty call
    assert R(cfg, 0, 8, None, None, None, None, None, None, 0, None) == OK  # empty batch: no pointer is read
    assert R(cfg, 4, 0, None, None, None, None, None, None, 1, None) == OK  # no steps
    for hole in range(6):                                                   # keys, actions, msgs, init, state, out
        args = [k, k, k, k, k, out]
        args[hole] = None
        assert R(cfg, 4, 8, *args, 0, None) == ENULL, hole
        assert b"null" in L.hftlob_last_error()
    for field in ("obs", "rewards", "done_all", "dones"):                   # the required outputs
        o = StepOut(k, k, k, k, None)
        setattr(o, field, None)
        assert R(cfg, 4, 8, k, k, k, k, k, C.byref(o), 1, None) == ENULL, field
        assert b"null output" in L.hftlob_last_error()


def test_launch_info_unchanged():
    """hftlob_launch_info keeps its seven fields: the selection it reports is this entry point's too"""
    assert [n for n, _ in _lib.LaunchInfo._fields_] == ["slot_sets", "nfix", "random_cancel", "rows_alias",
                                                        "lds_bytes", "tick_magic", "key_batch"]


def test_rollout_argument_checks_need_no_device():
    """MARLEnv.rollout's key checks raise before any device call"""
    import torch
    from hftlob.env import MARLEnv
    assert callable(MARLEnv.rollout)
    with pytest.raises(ValueError, match=r"\[T, E, 2\]"):
        MARLEnv.rollout(None, torch.zeros((4, 2), dtype=torch.int32), None, None, None)
    with pytest.raises(ValueError, match="T >= 1"):
        MARLEnv.rollout(None, torch.zeros((0, 4, 2), dtype=torch.int32), None, None, None)
