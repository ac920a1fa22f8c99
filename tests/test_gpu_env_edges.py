"""Env kernels at the book sizes the suite's other files never launch: the one-register-set
instantiations (k_env_step<1, 0, *>, k_env_reset<1>, k_env_rollout<1, 0, *>: nOrders, nTrades <= 64),
sizes on and across the 64-slot boundaries, the persistent general-size rollout
(k_env_rollout<S, 0, false>) and the persistent random-cancel rollout (k_env_rollout<S, 0, true>).
The comparisons are test_gpu_env's: every step against the CPU oracle (integers bit-exact, floats
within rtol = atol = 1e-5), the one-launch rollout against per-step launches and the oracle's
rollout loop; hftlob_env_launch_info asserts the instantiation each case launches."""
import dataclasses

import pytest

from book_edges import slot_sets
from hftlob.config_io import builtin_config
from test_gpu_env import quiet_rollout_parity, rollout_parity

pytestmark = pytest.mark.gpu


def _sized(name, nO, nT, **world):
    cfg = builtin_config(name)
    return dataclasses.replace(cfg, world_config=dataclasses.replace(cfg.world_config, nOrders=nO, nTrades=nT, **world))


STEP_SIZES = [("2_player_fq_fqc", nO, nT) for nO, nT in ((64, 64), (65, 64), (64, 65), (128, 128), (129, 100),
                                                          (100, 101), (16, 8), (24, 1))] + \
             [("3_player_fq_fqc_dir", 64, 64), ("3_player_fq_fqc_dir", 129, 100)]


@pytest.mark.parametrize("name,nO,nT", STEP_SIZES)
def test_env_step_parity_edge_sizes(name, nO, nT):
    """reset, sampled actions and 40 steps (state, obs, rewards, dones, info) at sizes on both sides of
    a register-set boundary, with either of nOrders / nTrades the larger, and at small books whose
    sides fill to their last row (16/8) and a one-row trade log (24/1)"""
    rollout_parity(_sized(name, nO, nT), E=16, K=40,
                   expect=dict(slot_sets=slot_sets(nO, nT), nfix=0, random_cancel=0))


ROLLOUT_SIZES = [("2_player_fq_fqc", 64, 64), ("2_player_fq_fqc", 128, 128), ("2_player_fq_fqc", 129, 100),
                 ("2_player_fq_fqc", 256, 256), ("3_player_fq_fqc_dir", 64, 64)]


@pytest.mark.parametrize("name,nO,nT", ROLLOUT_SIZES)
def test_persistent_rollout_general_sizes(name, nO, nT):
    """k_env_rollout<S, 0, false> for S = 1, 2, 4: one 70-step launch (the book resident in LDS, the
    quiet step body, an auto-reset inside) == 70 step_sampled launches and the oracle's rollout"""
    quiet_rollout_parity(_sized(name, nO, nT), E=24, T=70, nfix=0,
                         expect=dict(slot_sets=slot_sets(nO, nT), random_cancel=0))


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("nO,nT", [(100, 100), (64, 64)], ids=lambda v: str(v))
def test_persistent_rollout_random_cancel(nO, nT, mode):
    """k_env_rollout<S, 0, true> (cancel_mode 2 / 3) as ONE persistent launch (n_slices = 0) of 66
    steps: state, carried key and the last step's outputs == 66 step_sampled launches, end state
    and key == the oracle's rollout"""
    quiet_rollout_parity(_sized("2_player_fq_fqc", nO, nT, cancel_mode=mode), E=24, T=66, nfix=0,
                         expect=dict(slot_sets=slot_sets(nO, nT), random_cancel=1))
