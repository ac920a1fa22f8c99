"""The per-episode records of the evaluation launches (hftlob_env_rollout_eval_episodes,
hftlob_env_rollout_eval_drawn_episodes, hftlob_eval_tally_episodes) against their definition,
hftlob.evaluate.reduce_steps(max_episodes=) over one env.rollout(per_step=True) of the case: bit for bit
(equal, or both NaN), untouched slots included: every buffer starts filled with a sentinel.

The cases and their inputs are those of test_gpu_rollout_eval / test_gpu_rollout_actions.  The shipped
configs' episodes are at most 65 steps long, so T = 135 holds two episode ends per env and
a few steps of a third episode."""
import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.evaluate import Uniform
from test_gpu_env import MULTI_AGENT_CASES, _expect_launch, _multi_agent_config
from test_gpu_rollout_actions import NFIX, _same, _sized
from test_gpu_rollout_eval import FQ, _check_end, _eval_reference

pytestmark = pytest.mark.gpu
W = _lib.EPISODE_WORDS
SENTINEL = -12345.5
GUARD = 4 * W          # doubles after the buffer that no launch may touch
T2 = 135               # two episode ends and a bit


def _buffer(E, A, cap):
    """a sentinel-filled [E, A, cap, W] view at the front of a longer allocation, and the whole of it"""
    whole = torch.full((E * A * cap * W + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    return whole[:E * A * cap * W].view(E, A, cap, W), whole


def _eq(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _ref(V, cap, stats=None, t0=0, t1=None):
    """reduce_steps over the case's per-step outputs, from a sentinel buffer"""
    E, A = V["rew"].shape[1:]
    ep0 = torch.full((E, A, cap, W), SENTINEL, dtype=torch.float64, device="cuda")
    return EV.reduce_steps(V["rew"][t0:t1], V["words"][t0:t1], V["done"][t0:t1], V["env"].layout, stats=stats,
                           episodes=ep0)


def _fq_case(E=5):
    V = _eval_reference("fq_fqc", builtin_config(FQ), E, T2)
    _expect_launch(V["env"], NFIX)
    assert bool((V["done"].sum(dim=0) == 2).all()), "two episode ends per env"
    return V


@pytest.mark.parametrize("cap", [3, 2, 1])
def test_resident_kernel_two_ends(cap):
    """k_env_rollout_eval<2, 100, false, false>, E = 5, T = 135.  cap 3: slot 2 stays the sentinel; cap 2: an
    exact fit; cap 1: the second record is dropped (word 1 = 2 > cap) and nothing lands in the next row
    or past the buffer.  Stats, end state and last-step outputs are the launch's without records."""
    V = _fq_case()
    env, params, E, A = V["env"], V["params"], 5, V["env"].num_agents
    ep, whole = _buffer(E, A, cap)
    s = V["start"].clone(env)
    out = env.rollout_eval(V["keys"], s, V["acts"], params, episodes=ep)
    torch.cuda.synchronize()
    assert len(out) == 7 and out[6] is ep
    stats = out[5]
    rst, rep = _ref(V, cap)
    assert _eq(ep, rep), torch.nonzero(~((ep == rep) | (ep.isnan() & rep.isnan())))[:8].tolist()
    assert bool((whole[-GUARD:] == SENTINEL).all()), "nothing is written past the buffer"
    assert _eq(stats, V["ref"]) and _eq(stats, rst) and bool((stats[:, :, 1] == 2).all())
    n = min(cap, 2)
    assert not bool((ep[:, :, :n] == SENTINEL).any()) and bool((ep[:, :, n:] == SENTINEL).all())
    ends = torch.nonzero(V["done"].t())[:, 1].view(E, 2).to(torch.float64)        # each env's two last steps
    assert torch.equal(ep[:, 0, 0, 1], ends[:, 0] + 1) and (cap < 2 or torch.equal(ep[:, 1, 1, 1], ends[:, 1] - ends[:, 0]))
    # the record is what the accumulators added: with both ends kept, their sums are words 4 and 58 + 2k
    if cap >= 2:
        assert torch.equal(ep[:, :, 0, 0] + ep[:, :, 1, 0], stats[:, :, 4])
        fin = ~(ep[:, :, :2, 2:].isnan().any(dim=2))
        assert torch.equal((ep[:, :, 0, 2:] + ep[:, :, 1, 2:])[fin], stats[:, :, 58::2][fin])
    _check_end("episodes", V, s, out[0], out[2], out[3], env)
    # the existing entry point over the same inputs: the same stats, state and outputs
    s0 = V["start"].clone(env)
    old = env.rollout_eval(V["keys"], s0, V["acts"], params)
    assert len(old) == 6 and _eq(old[5], stats) and bool((s0.buf == s.buf).all())
    assert _same(old[0], out[0]) and _same(old[2], out[2])


def test_chunked_launches_carry_stats_and_episodes():
    """33 + 37 + 65 steps (the cuts before, and exactly at, an episode end) equal one call"""
    V = _fq_case()
    env, params = V["env"], V["params"]
    ep, whole = _buffer(5, env.num_agents, 3)
    s, stats, t0 = V["start"].clone(env), None, 0
    for n in (33, 37, 65):
        out = env.rollout_eval(V["keys"][t0:t0 + n], s, V["acts"][t0:t0 + n], params, stats=stats, episodes=ep)
        assert out[6] is ep and (stats is None or out[5] is stats)
        stats, t0 = out[5], t0 + n
    rst, rep = _ref(V, 3)
    assert _eq(ep, rep) and _eq(stats, rst) and bool((whole[-GUARD:] == SENTINEL).all())
    assert bool((s.buf == V["end"]).all())


def test_a_start_from_word_1_of_1_writes_at_indices_1_and_2():
    V = _fq_case()
    env, params = V["env"], V["params"]
    ep, _ = _buffer(5, env.num_agents, 3)
    stats = torch.zeros((5, env.num_agents, 106), dtype=torch.float64, device="cuda")
    stats[:, :, 1] = 1.0
    rst, rep = _ref(V, 3, stats=stats)
    env.rollout_eval(V["keys"], V["start"].clone(env), V["acts"], params, stats=stats, episodes=ep)
    assert _eq(ep, rep) and _eq(stats, rst) and bool((stats[:, :, 1] == 3).all())
    assert bool((ep[:, :, 0] == SENTINEL).all()) and not bool((ep[:, :, 1:] == SENTINEL).any())


_MA = MULTI_AGENT_CASES[1]
assert _MA[0] == "3_player_fq_fqc_dir"


@pytest.mark.parametrize("tag,cfg,expect", [
    ("sized_64_64", lambda: _sized(FQ, 64, 64), dict(slot_sets=1, nfix=0, random_cancel=0)),
    ("rc2", lambda: _sized(FQ, 64, 64, cancel_mode=2), dict(slot_sets=1, nfix=0, random_cancel=1)),
    ("multi_3_player", lambda: _multi_agent_config(*_MA), None),
], ids=["general_1_set", "random_cancel", "three_types_7_agents"])
def test_other_instantiations(tag, cfg, expect):
    """the general one-slot-set kernel, the random-cancel one, and the 3-type config with [2, 2, 3] agents:
    T just past two episode ends, cap 2 with every slot written"""
    E = 6
    V = _eval_reference(tag, cfg(), E, T2)
    env, params = V["env"], V["params"]
    _expect_launch(env, expect)
    assert bool((V["done"].sum(dim=0) == 2).all())
    ep, whole = _buffer(E, env.num_agents, 2)
    s = V["start"].clone(env)
    out = env.rollout_eval(V["keys"], s, V["acts"], params, episodes=ep)
    rst, rep = _ref(V, 2)
    assert _eq(ep, rep), torch.nonzero(~((ep == rep) | (ep.isnan() & rep.isnan())))[:8].tolist()
    assert _eq(out[5], rst) and bool((whole[-GUARD:] == SENTINEL).all()) and not bool((ep == SENTINEL).any())
    _check_end(tag, V, s, out[0], out[2], out[3], env)


def test_drawn_launch_equals_the_launch_over_its_actions():
    V = _fq_case()
    env, params, E = V["env"], V["params"], 5
    n_types = len(env.multi_agent_config.number_of_agents_per_type)
    masks = EV.draw_masks(env, EV.policy_entries([Uniform.all()] * n_types, n_types), fixed_too=True)
    dk = (torch.arange(T2 * n_types * 2, dtype=torch.int32, device="cuda") * 7919 + 11).view(T2, n_types, 2)
    acts = torch.full((T2, E, env.action_words), -1, dtype=torch.int32, device="cuda")
    ep_d, whole = _buffer(E, env.num_agents, 3)
    s = V["start"].clone(env)
    d = env.rollout_eval_drawn(V["keys"], s, dk, masks, params, actions_out=acts, episodes=ep_d)
    assert len(d) == 7 and d[6] is ep_d and bool((acts >= 0).all())
    assert len(acts.unique()) > 2, "the actions are drawn"
    ep_a, _ = _buffer(E, env.num_agents, 3)
    s2 = V["start"].clone(env)
    a = env.rollout_eval(V["keys"], s2, acts, params, episodes=ep_a)
    assert _eq(ep_d, ep_a) and _eq(d[5], a[5]) and bool((s.buf == s2.buf).all())
    assert bool((whole[-GUARD:] == SENTINEL).all()) and bool((ep_d[:, :, 2] == SENTINEL).all())
    assert not bool((ep_d[:, :, :2] == SENTINEL).any())
    s3 = V["start"].clone(env)
    old = env.rollout_eval_drawn(V["keys"], s3, dk, masks, params)
    assert len(old) == 6 and _eq(old[5], d[5]) and bool((s3.buf == s.buf).all())


@pytest.mark.parametrize("tag,cfg,E", [("fq_fqc", lambda: builtin_config(FQ), 11),
                                       ("3_player", lambda: builtin_config("3_player_fq_fqc_dir"), 7)],
                         ids=["E11_A2", "E7_A3"])
def test_tally_steps_one_call_and_a_call_per_step(tag, cfg, E):
    """hftlob_eval_tally_episodes over the case's per-step outputs, 2 x 11 and 3 x 7 agents (more than
    one 256-lane workgroup): one call of T = 135, and 135 calls of T = 1 as evaluate_policy makes them.
    Both equal reduce_steps and the records of the rollout launch."""
    V = _eval_reference(tag, cfg(), E, T2)
    env, params, A = V["env"], V["params"], V["env"].num_agents
    assert E * A * 25 > 256 and bool((V["done"].sum(dim=0) == 2).all())
    rst, rep = _ref(V, 3)
    ep1, whole1 = _buffer(E, A, 3)
    st1, got = EV.tally_steps(V["rew"], V["words"], V["done"], env.layout, episodes=ep1)
    assert got is ep1 and _eq(ep1, rep) and _eq(st1, rst) and bool((whole1[-GUARD:] == SENTINEL).all())
    epn, wholen = _buffer(E, A, 3)
    stn = torch.zeros_like(st1)
    for t in range(T2):
        EV.tally_steps(V["rew"][t:t + 1], V["words"][t:t + 1], V["done"][t:t + 1], env.layout, stats=stn, episodes=epn)
    assert _eq(epn, rep) and _eq(stn, rst) and bool((wholen[-GUARD:] == SENTINEL).all())
    epr, _ = _buffer(E, A, 3)
    env.rollout_eval(V["keys"], V["start"].clone(env), V["acts"], params, episodes=epr)
    assert _eq(epr, ep1)
    # cap 1 drops the second record here too
    epc, wholec = _buffer(E, A, 1)
    stc, _ = EV.tally_steps(V["rew"], V["words"], V["done"], env.layout, episodes=epc)
    assert _eq(epc, _ref(V, 1)[1]) and bool((stc[:, :, 1] == 2).all()) and bool((wholec[-GUARD:] == SENTINEL).all())
    # without a buffer: the stats tensor alone, the same bits
    assert _eq(EV.tally_steps(V["rew"], V["words"], V["done"], env.layout), rst)


@pytest.fixture(scope="module")
def env_info():
    from test_gpu_policy_rollout import make_env
    return make_env(True)


def test_evaluators_return_logs(env_info):
    """evaluate_policy (a tally launch per step) against evaluate_baseline (the drawn launch) on fixed
    entries, and with a net that always takes the same action: the same stats, so the same records."""
    from test_gpu_policy_rollout import _constant_nets
    env, E, T, seed = env_info, 4, 70, 5
    acts = [4, 2]
    ev_b, log_b = EV.evaluate_baseline(env, acts, E, T, seed, chunk=32, max_episodes=4)
    ev_f, log_f = EV.evaluate_fixed_actions(env, acts, E, T, seed, chunk=32, max_episodes=4)
    ev_p, log_p = EV.evaluate_policy(env, acts, E, T, seed, greedy=True, chunk=32, max_episodes=4)
    _, fixed = _constant_nets(env, acts)
    ev_n, log_n = EV.evaluate_policy(env, [fixed[0], acts[1]], E, T, seed, greedy=True, chunk=32, max_episodes=4)
    for ev, log in ((ev_f, log_f), (ev_p, log_p), (ev_n, log_n)):
        assert torch.equal(ev.stats, ev_b.stats)
        assert torch.equal(log.count, log_b.count) and log.dropped == 0
        assert _eq(log.rewards(), log_b.rewards()) and torch.equal(log.lengths(), log_b.lengths())
        assert _eq(log.field(1, "drift"), log_b.field(1, "drift"))
    assert len(log_b) == E and tuple(log_b.rewards().shape) == (E, 2)
    assert torch.equal(log_b.lengths(), ev_b.stats[:, 0, 6].cpu()) and bool((log_b.lengths() > 60).all())
    assert torch.equal(log_b.rewards(), ev_b.stats[:, :, 4].cpu()), "one episode per env: its sum is word 4"
    assert isinstance(EV.evaluate_policy(env, acts, E, 8, seed), EV.EvalStats)
    nets, _ = _constant_nets(env, acts)
    combos = EV.evaluate_combinations(env, nets, acts, E, T, seed, max_episodes=4)
    assert list(combos) == ["BB", "BL", "LB", "LL"]
    for desc, (ev, log) in combos.items():
        assert isinstance(ev, EV.EvalStats) and tuple(log.rewards().shape) == (E, 2) and log.cap == 4
    assert _eq(combos["BB"][1].rewards(), log_b.rewards())


def test_refused_buffers():
    V = _fq_case()
    env, params, E, A = V["env"], V["params"], 5, V["env"].num_agents
    good = torch.zeros((E, A, 2, W), dtype=torch.float64, device="cuda")
    stats = torch.full((E, A, 106), 3.0, dtype=torch.float64, device="cuda")
    s = V["start"].clone(env)
    bad = [torch.zeros((E, A, 0, W), dtype=torch.float64, device="cuda"),         # cap 0
           good.cpu(), good.float(), good[:, :, :, :W - 1], good[:4], good.reshape(E, A, 2 * W),
           torch.zeros((E, A, 2, 2 * W), dtype=torch.float64, device="cuda")[:, :, :, :W],   # not contiguous
           good.permute(0, 1, 3, 2)]
    n_types = len(env.multi_agent_config.number_of_agents_per_type)
    masks = EV.draw_masks(env, EV.policy_entries([Uniform.all()] * n_types, n_types), fixed_too=True)
    dk = torch.zeros((T2, n_types, 2), dtype=torch.int32, device="cuda")
    for ep in bad:
        with pytest.raises(ValueError, match="ep_cap"):
            env.rollout_eval(V["keys"], s, V["acts"], params, stats=stats, episodes=ep)
        with pytest.raises(ValueError, match="ep_cap"):
            env.rollout_eval_drawn(V["keys"], s, dk, masks, params, stats=stats, episodes=ep)
        with pytest.raises(ValueError, match="ep_cap"):
            EV.tally_steps(V["rew"], V["words"], V["done"], env.layout, stats=stats, episodes=ep)
    torch.cuda.synchronize()
    assert bool((s.buf == V["start"].buf).all()) and bool((stats == 3.0).all()), "a refused call launches nothing"
    # the ABI's own refusals (never launched): a NULL buffer and a cap < 1
    L, k = _lib.lib(), _lib.ptr(good)
    m = (_lib.C.c_uint32 * A)(*([0] * A))
    for episodes, cap in ((None, 2), (k, 0), (k, -1)):
        assert L.hftlob_eval_tally_episodes(E, A, 1, env.layout.info_words, k, k, k, m, k, episodes, cap, None) == -1
    with pytest.raises(ValueError, match="ep_cap"):
        EV.evaluate_fixed_actions(env, [4, 2], 4, 8, 0, max_episodes=0)
