"""The baked-config instantiations of the persistent sampled rollout (k_env_rollout's BAKED
parameter, hftlob.hip) against the general kernel and the CPU oracle, bit for bit (floats are
compared as their int32 words).

Baked against general, and against the oracle: the config, 5 envs, 70 steps from the reset state of
generate_day(n_msgs=20_000, seed=8) (an episode of the day's windows is 64 steps, so the launch
crosses the episode end and the auto-reset inside its quiet loop).  rollout_sampled runs with
per_step False and True (n_slices = 0), each once with the switch hftlob_set_baked on and once with
it off: end state, carried key and outputs (per_step: every step's) are equal between the two runs,
and the baked run's end state and key equal oracle.pyoracle.rollout_sampled.  The same with a shard
(key_e0 = 3, key_n = 11, 4 envs).  baked_id() >= 0 is asserted in the baked runs and == -1 with the
switch off (the launch code takes the baked kernel exactly for baked_id() >= 0: env_variant).

Fallback on mismatch: a day generated on tick 25 (with the config's tick_size 25), and separately
fixed_quant_value + 1 on the first agent type: baked_id() == -1 and a 10-step rollout equals the
oracle."""
import dataclasses

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day

T = 70
BAKED = {"2_player_fq_fqc": 0, "3_player_fq_fqc_dir": 1}     # the ids the library has kernels for
KEY_BATCH = {"2_player_fq_fqc": 1, "3_player_fq_fqc_dir": 0}  # each one's key-batch mode (its kernel's KB)
_REF = {}


def _env(name):
    from hftlob.env import MARLEnv
    if name not in _REF:
        cfg = builtin_config(name)
        w = cfg.world_config
        day = generate_day(n_msgs=20_000, seed=8, snap_every=w.n_data_msg_per_step * w.start_resolution)
        _REF[name] = (MARLEnv(None, cfg, data=day), day)
    return _REF[name]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def _words(x):
    """every tensor of a (nested) output as int32 / uint8 words on the host, in a fixed order"""
    if isinstance(x, torch.Tensor):
        a = x.detach().cpu().contiguous().numpy()
        return [a.view(np.int32) if a.dtype == np.float32 else a]
    if isinstance(x, dict):
        return [w for k in sorted(x, key=str) for w in _words(x[k])]
    if isinstance(x, (list, tuple)):
        return [w for v in x for w in _words(v)]
    return []


def _run(env, E, n_steps, per_step, e0, n, baked):
    """reset + one persistent rollout_sampled launch with the switch set to `baked`"""
    params = env.default_params
    k0 = np.arange(2 * E, dtype=np.uint32).reshape(E, 2) + 3
    prev = _lib.set_baked(baked)
    try:
        bid = env.baked_id()
        _, state = env.reset(_dev(k0), params)
        start = state.buf.cpu().numpy().copy()
        k_in = _dev(np.array([0, 7], np.uint32))
        k_out = torch.empty_like(k_in)
        acts = torch.zeros((n_steps, E, env.action_words) if per_step else (E, env.action_words), dtype=torch.int32,
                           device="cuda")
        obs, state, rew, dones, info = env.rollout_sampled(k_in, k_out, state, params, n_steps, per_step=per_step,
                                                           actions_out=acts, n_slices=0, key_e0=e0, key_n=n)
        torch.cuda.synchronize()
    finally:
        _lib.set_baked(prev)
    out = _words([obs, rew, dones, info, acts])
    return bid, start, state.buf.cpu().numpy().copy(), k_out.cpu().numpy().view(np.uint32).copy(), out


def _baked_vs_general(name, E, e0, n):
    from oracle import pyoracle as O
    env, day = _env(name)
    info = env.launch_info()
    assert (info["slot_sets"], info["nfix"], info["random_cancel"], info["rows_alias"], info["key_batch"]) == \
        (2, 100, 0, 0, KEY_BATCH[name]), info                       # the variant the baked kernels exist for
    init = env._init_states.cpu().numpy()
    for per_step in (False, True):
        bid, start, st_b, key_b, out_b = _run(env, E, T, per_step, e0, n, True)
        assert bid == BAKED[name], "the launch takes the baked kernel"
        gid, start_g, st_g, key_g, out_g = _run(env, E, T, per_step, e0, n, False)
        assert gid == -1, "switch off: the launch takes the general kernel"
        assert (start == start_g).all()
        assert (st_b == st_g).all(), f"per_step={per_step}: end state differs at {np.argwhere(st_b != st_g)[:5].tolist()}"
        assert (key_b == key_g).all(), f"per_step={per_step}: carried key"
        assert len(out_b) == len(out_g) and len(out_b) >= 5
        for i, (a, b) in enumerate(zip(out_b, out_g)):
            assert a.shape == b.shape and (a == b).all(), f"per_step={per_step}: output {i} differs"
        o_st, o_key = O.rollout_sampled(env.cfg_c, np.array([0, 7], np.uint32), day.msgs, init, start, T,
                                        key_e0=e0, key_n=n)
        assert (o_st[:, env.layout.off_loaded + 5] < T).all(), "every env crossed an episode end"
        assert (st_b == o_st).all(), f"per_step={per_step}: baked end state differs from the oracle"
        assert (key_b == o_key).all(), f"per_step={per_step}: baked carried key differs from the oracle"


@pytest.mark.gpu
def test_baked_equals_general_and_oracle():
    _baked_vs_general("2_player_fq_fqc", 5, 0, 5)


@pytest.mark.gpu
def test_baked_equals_general_and_oracle_shard():
    _baked_vs_general("2_player_fq_fqc", 4, 3, 11)


@pytest.mark.gpu
def test_baked_equals_general_and_oracle_c5():
    _baked_vs_general("3_player_fq_fqc_dir", 5, 0, 5)


def _fallback(cfg, day):
    from hftlob.env import MARLEnv
    from oracle import pyoracle as O
    env = MARLEnv(None, cfg, data=day)
    assert env.baked_id() == -1
    E, n_steps = 5, 10
    bid, start, st, key, _ = _run(env, E, n_steps, False, 0, E, True)
    assert bid == -1
    o_st, o_key = O.rollout_sampled(env.cfg_c, np.array([0, 7], np.uint32), day.msgs, env._init_states.cpu().numpy(),
                                    start, n_steps)
    assert (st == o_st).all() and (key == o_key).all()


@pytest.mark.gpu
def test_fallback_other_tick():
    cfg = builtin_config("2_player_fq_fqc")
    w = dataclasses.replace(cfg.world_config, tick_size=25)
    cfg = dataclasses.replace(cfg, world_config=w)
    day = generate_day(n_msgs=20_000, seed=8, tick=25, snap_every=w.n_data_msg_per_step * w.start_resolution)
    _fallback(cfg, day)


@pytest.mark.gpu
def test_fallback_other_quant():
    cfg = builtin_config("2_player_fq_fqc")
    name, t0 = next(iter(cfg.dict_of_agents_configs.items()))
    agents = dict(cfg.dict_of_agents_configs)
    agents[name] = dataclasses.replace(t0, fixed_quant_value=t0.fixed_quant_value + 1)
    cfg = dataclasses.replace(cfg, dict_of_agents_configs=agents)
    _fallback(cfg, _env("2_player_fq_fqc")[1])
