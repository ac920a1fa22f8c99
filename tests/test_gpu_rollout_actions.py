"""MARLEnv.rollout / hftlob_env_rollout_actions (k_env_rollout_actions: T steps with the caller's
keys and actions in one persistent launch) against T env.step launches over the same inputs and
against the CPU oracle's step loop.

Every case: reset E envs, keys [T, E, 2] from a split_keys chain (every step's keys differ),
actions [T] from env.sample_actions(keys[t]); path A is T env.step calls, path B one env.rollout
call, the oracle loops O.env_step on the CPU.  B's end state equals A's bit for bit (the same
device code under -ffp-contract=off) and the oracle's with test_gpu_env's _compare_state (integers
exact, floats within 1e-5); with per_step every step's obs / rewards / dones / info equal A's bit
for bit, without it the last step's do.  hftlob_env_launch_info names the instantiation, and a case
that claims an auto-reset inside the launch asserts one (step_counter < T for every env, on the
oracle's state too)."""
import dataclasses

import numpy as np
import pytest
import torch

from book_edges import slot_sets
from hftlob.config_io import builtin_config
from hftlob.env import MARLEnv, split_keys
from oracle import pyoracle as O
from test_gpu_env import (MULTI_AGENT_CASES, _compare_state, _day, _expect_launch, _multi_agent_config,
                          speed_test_config)

pytestmark = pytest.mark.gpu


def _sized(name, nO, nT, **world):
    cfg = builtin_config(name)
    return dataclasses.replace(cfg, world_config=dataclasses.replace(cfg.world_config, nOrders=nO, nTrades=nT, **world))


def _rows_alias_config():
    """the `default` config (MM bobRL + EXE fixed_quants_complex) with [5, 5] agents: 60 agent message
    rows, which the 100/100 kernel keeps inside the trade log"""
    return dataclasses.replace(builtin_config("default"), number_of_agents_per_type=[5, 5])


_REF = {}


def _reference(tag, cfg, E, T):
    """The case's inputs, path A (T env.step launches) and the oracle's end state: computed once per
    case, shared by its per_step variants, never modified (path B runs on clones)."""
    key = (tag, E, T)
    if key in _REF:
        return _REF[key]
    w = cfg.world_config
    day = _day(w, 2_000_000)
    env = MARLEnv(None, cfg, data=day)
    params = env.default_params
    k0 = torch.from_numpy(np.arange(2 * E, dtype=np.uint32).reshape(E, 2).view(np.int32)).cuda()
    _, state = env.reset(k0, params)
    start = state.clone(env)
    keys = torch.empty((T, E, 2), dtype=torch.int32, device="cuda")
    acts = torch.empty((T, E, env.action_words), dtype=torch.int32, device="cuda")
    rng = k0
    for t in range(T):
        nk = split_keys(rng, 2)
        rng = nk[:, 0].contiguous()
        keys[t] = nk[:, 1]
        acts[t] = env.sample_actions(keys[t])
    assert len({keys[t].cpu().numpy().tobytes() for t in range(T)}) == T, "every step's keys differ"
    steps = []
    for t in range(T):
        obs, state, rew, dones, _ = env.step(keys[t], state, acts[t], params)
        steps.append(dict(obs=[x.clone() for x in obs], rew=[x.clone() for x in rew], done=dones["__all__"].clone(),
                          dones=[x.clone() for x in dones["agents"]], info=env.last_info_words.clone()))
    init = env._init_states.cpu().numpy()
    st = start.buf.cpu().numpy().copy()
    kn, an = keys.cpu().numpy().view(np.uint32), acts.cpu().numpy()
    for t in range(T):
        st = O.env_step(env.cfg_c, kn[t], an[t], day.msgs, init, st)[0]
    _compare_state(env, st, state.buf.cpu().numpy(), f"{tag}: per-step launches vs oracle")
    _REF[key] = dict(env=env, params=params, start=start, keys=keys, acts=acts, steps=steps, end=state.buf.clone(),
                     oracle=st)
    return _REF[key]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(a, b))


def _check_step(tag, t, ref, obs, rew, dones, info):
    assert _same(obs, ref["obs"]), f"{tag} step {t}: obs"
    assert _same(rew, ref["rew"]), f"{tag} step {t}: rewards"
    assert bool((dones["__all__"] == ref["done"]).all()), f"{tag} step {t}: done_all"
    assert _same(dones["agents"], ref["dones"]), f"{tag} step {t}: dones"
    assert bool((info == ref["info"]).all()), f"{tag} step {t}: info"


def rollout_actions_parity(tag, cfg, E, T, per_step, expect=None, reset_inside=False):
    R = _reference(tag, cfg, E, T)
    env, params = R["env"], R["params"]
    _expect_launch(env, expect)
    s2 = R["start"].clone(env)
    obs, s_ret, rew, dones, info = env.rollout(R["keys"], s2, R["acts"], params, per_step=per_step)
    torch.cuda.synchronize()
    assert s_ret is s2, "the state is updated in place"
    bad = torch.nonzero(s2.buf != R["end"])
    assert bad.numel() == 0, f"{tag}: end state vs per-step launches (env, word) {bad[:5].tolist()}"
    _compare_state(env, R["oracle"], s2.buf.cpu().numpy(), f"{tag}: rollout vs oracle")
    words = env.last_info_words
    if per_step:
        assert obs[0].shape[:2] == (T, E) and rew[0].shape[:2] == (T, E) and dones["__all__"].shape == (T, E)
        assert words.shape[0] == T * E and info["world"]["step_counter"].shape[0] == T * E
        words = words.reshape(T, E, -1)
        for t in range(T):
            _check_step(tag, t, R["steps"][t], [x[t] for x in obs], [x[t] for x in rew],
                        {"__all__": dones["__all__"][t], "agents": [x[t] for x in dones["agents"]]}, words[t])
    else:
        assert obs[0].shape[0] == E and dones["__all__"].shape == (E,)
        _check_step(tag, T - 1, R["steps"][T - 1], obs, rew, dones, words)
    if reset_inside:
        L = env.layout
        assert (R["oracle"][:, L.off_loaded + 5] < T).all(), "oracle: every env crossed its episode end"
        assert (s2.world_state.step_counter.cpu().numpy() < T).all(), "every env crossed its episode end"


NFIX = dict(slot_sets=2, nfix=100, random_cancel=0, rows_alias=0)


@pytest.mark.parametrize("per_step", [False, True])
def test_resident_kernel_crosses_reset(per_step):
    """k_env_rollout_actions<2, 100, false, false>: 70 steps from the reset state cross every env's
    episode end (65-step episodes), so the book is resident in LDS, dropped at the auto-reset and
    reloaded from the record; per_step = False runs steps 0..68 in the quiet body"""
    rollout_actions_parity("fq_fqc", builtin_config("2_player_fq_fqc"), 24, 70, per_step, expect=NFIX,
                           reset_inside=True)


@pytest.mark.parametrize("E,T,per_step", [(8, 1, False), (8, 1, True), (1, 1, False), (1, 5, False), (1, 5, True),
                                          (1025, 3, False), (1025, 3, True)])
def test_single_step_and_single_env(E, T, per_step):
    """T = 1: the emitting loop alone, keep = false on the only step; E = 1: a one-workgroup launch;
    E = 1025: the smallest launch whose waves rank their issue priority, after steps 0 and 1 of T = 3"""
    rollout_actions_parity("fq_fqc", builtin_config("2_player_fq_fqc"), E, T, per_step, expect=NFIX)


@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("nO,nT", [(64, 64), (128, 128), (129, 100)], ids=lambda v: str(v))
def test_general_sizes(nO, nT, per_step):
    """k_env_rollout_actions<S, 0, false> for S = 1, 2, 4"""
    rollout_actions_parity(f"sized_{nO}_{nT}", _sized("2_player_fq_fqc", nO, nT), 16, 40, per_step,
                           expect=dict(slot_sets=slot_sets(nO, nT), nfix=0, random_cancel=0, rows_alias=0))


@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("mode", [2, 3])
def test_random_cancel(mode, per_step):
    """k_env_rollout_actions<1, 0, true>: the cancel_mode 2 / 3 draws come from the caller's step keys"""
    rollout_actions_parity(f"rc{mode}", _sized("2_player_fq_fqc", 64, 64, cancel_mode=mode), 16, 40, per_step,
                           expect=dict(slot_sets=1, nfix=0, random_cancel=1))


@pytest.mark.parametrize("per_step", [False, True])
def test_rows_alias(per_step):
    """k_env_rollout_actions<2, 100, false, true>: the agent rows inside the trade log"""
    rollout_actions_parity("rows_alias", _rows_alias_config(), 16, 40, per_step,
                           expect=dict(slot_sets=2, nfix=100, random_cancel=0, rows_alias=1))


def test_rows_alias_crosses_reset():
    """the rows-alias kernel over Speed_test's 32-step episodes: 40 steps cross every env's episode
    end in the quiet loop, so its resident book is dropped and reloaded (test_gpu_env's
    test_speed_test_rows_alias_persistent relies on the same episodes at 70 steps)"""
    rollout_actions_parity("rows_alias_32", speed_test_config([5, 5], 100), 16, 40, False,
                           expect=dict(slot_sets=2, nfix=100, random_cancel=0, rows_alias=1), reset_inside=True)


def test_general_size_crosses_reset():
    """a general-size kernel (no resident book) with an auto-reset inside its quiet loop: 64/64 slots,
    70 steps over 65-step episodes (test_gpu_env_edges' persistent rollout at this size and length)"""
    rollout_actions_parity("sized_64_64", _sized("2_player_fq_fqc", 64, 64), 16, 70, False,
                           expect=dict(slot_sets=1, nfix=0, random_cancel=0), reset_inside=True)


@pytest.mark.parametrize("per_step", [False, True])
def test_multidiscrete_fixed_prices(per_step):
    """EXE fixed_prices with [2, 3] agents: 3 MultiDiscrete action words per EXE agent, read by lanes
    0..2 of the general-size kernel (fixed_prices configs never take the 100/100 one)"""
    name, agents, changes = MULTI_AGENT_CASES[2]
    assert changes["action_space"] == "fixed_prices"
    cfg = _multi_agent_config(name, agents, changes)
    R = _reference("fixed_prices", cfg, 16, 40)
    assert R["env"].action_words == 2 + 3 * 3
    rollout_actions_parity("fixed_prices", cfg, 16, 40, per_step, expect=dict(slot_sets=2, nfix=0, random_cancel=0))


@pytest.mark.parametrize("per_step", [False, True])
def test_three_agent_types(per_step):
    rollout_actions_parity("3_player", builtin_config("3_player_fq_fqc_dir"), 16, 40, per_step, expect=NFIX)


def test_per_type_actions_and_bad_arguments():
    """the per-type list step accepts, with a leading T ([T, E, n_t] Discrete, [T, E, n_t, width]
    MultiDiscrete), gives the flat tensor's result; shapes and dtypes that disagree raise ValueError"""
    name, agents, changes = MULTI_AGENT_CASES[2]
    E, T = 6, 5
    R = _reference("fixed_prices", _multi_agent_config(name, agents, changes), E, T)
    env, params, keys, acts = R["env"], R["params"], R["keys"], R["acts"]
    W = env.action_words
    per_type = [acts[:, :, :2].contiguous(), acts[:, :, 2:].reshape(T, E, 3, 3).contiguous()]
    for t in range(T):  # the list is step's list with a leading T
        assert _same([x[t] for x in per_type], env.split_actions(acts[t]))
    s_flat, s_list = R["start"].clone(env), R["start"].clone(env)
    o1, _, r1, d1, _ = env.rollout(keys, s_flat, acts, params, per_step=True)
    o1, r1, da1 = [x.clone() for x in o1], [x.clone() for x in r1], d1["__all__"].clone()
    o2, _, r2, d2, _ = env.rollout(keys.view(torch.uint32), s_list, per_type, params, per_step=True)
    assert bool((s_flat.buf == s_list.buf).all()) and bool((s_flat.buf == R["end"]).all())
    assert _same(o1, o2) and _same(r1, r2) and bool((da1 == d2["__all__"]).all())
    s = R["start"].clone(env)
    before = s.buf.clone()
    bad = [(keys, acts[:-1]),                                  # T disagrees
           (keys, acts[:, :-1]),                               # E disagrees
           (keys, acts[:, :, :-1].contiguous()),               # action_words disagrees
           (keys, acts.reshape(T * E, W)),                     # no leading T
           (keys, acts.to(torch.int64)),                       # dtype
           (keys, acts.to(torch.float32)),
           (keys, [per_type[0]]),                              # a type missing
           (keys, [per_type[0], per_type[1].reshape(T, E, 9)]),   # MultiDiscrete without its width axis
           (keys, [per_type[0][:, :, :1], per_type[1]]),       # n_t disagrees
           (keys, [per_type[0].to(torch.int64), per_type[1]]),
           (keys[0], acts[0]),                                 # step's [E, 2] keys
           (keys[:0], acts[:0]),                               # T < 1
           (keys.to(torch.int64), acts),
           (keys[:, :-1], acts)]                               # the state holds E envs
    for k, a in bad:
        with pytest.raises(ValueError):
            env.rollout(k, s, a, params)
    torch.cuda.synchronize()
    assert bool((s.buf == before).all()), "a refused call launches nothing"


def test_graph_capture():
    """env.rollout captured in a HIP graph on one stream with static key, action and state tensors;
    two replays with new actions written in place between them, each equal to the per-step path"""
    cfg = builtin_config("2_player_fq_fqc")
    E, T = 16, 8
    R = _reference("fq_fqc", cfg, E, T)
    env = MARLEnv(None, cfg, data=_day(cfg.world_config, 2_000_000), persistent_outputs=True)
    params = env.default_params
    # the second replay's actions: drawn from other keys than the steps' own
    acts_b = torch.stack([env.sample_actions(R["keys"][(t + 3) % T]) for t in range(T)])
    assert not bool((acts_b == R["acts"]).all())
    s_b = R["start"].clone(env)
    for t in range(T):
        env.step(R["keys"][t], s_b, acts_b[t], params)
    gk, ga, gs = R["keys"].clone(), R["acts"].clone(), R["start"].clone(env)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (module load, output buffers)
        env.rollout(gk, gs, ga, params)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.rollout(gk, gs, ga, params)
    for acts, want, tag in ((R["acts"], R["end"], "first"), (acts_b, s_b.buf, "second")):
        gs.buf.copy_(R["start"].buf)
        ga.copy_(acts)
        g.replay()
        torch.cuda.synchronize()
        assert bool((gs.buf == want).all()), f"{tag} replay: end state"
    assert not bool((R["end"] == s_b.buf).all()), "the two action sets lead to different states"
