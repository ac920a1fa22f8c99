"""hftlob.evaluate on the CPU: reduce_steps (the definition hftlob_env_rollout_eval's accumulators
are held to) on a hand-written example, EvalStats against numpy, chunked reduction, and the
several-actions-per-type refusal.

The example: T = 4 steps, E = 2 envs, one MM agent; env 0's episode ends at step 1, env 1's never.
Info word k of env e at step t holds c_k + t + 8 e, with c_k = (k + 1) / 2 for the float32 words of
layout.INFO_MM and k + 1 for its int32 words: every value, sum and square below is exact."""
import math
import types

import numpy as np
import pytest
import torch

from hftlob import evaluate as EV
from hftlob.layout import AGENT_MM, INFO_AGENT_WORDS, INFO_MM, INFO_WORLD_WORDS

T, E = 4, 2
LAYOUT = types.SimpleNamespace(agent_kinds=[AGENT_MM], agent_types=[0],
                               info_words=INFO_WORLD_WORDS + INFO_AGENT_WORDS)
REWARDS = [[1.5, -0.5, 2.0, 0.25],      # env 0: the episode ends after 1.5 - 0.5; 2.0 + 0.25 is the running one
           [0.5, 0.5, -1.0, 3.0]]       # env 1
DONE = [[False, True, False, False], [False, False, False, False]]


def _c(k):
    return (k + 1) / 2 if INFO_MM[k][1] else float(k + 1)


def _value(e, k, t):
    return _c(k) + t + 8 * e


def _example():
    rew = torch.tensor(REWARDS, dtype=torch.float32).t().reshape(T, E, 1).contiguous()
    done = torch.tensor(DONE).t().contiguous()
    info = torch.full((T, E, LAYOUT.info_words), 77, dtype=torch.int32)     # the world words are never read
    for t in range(T):
        for e in range(E):
            for k in range(INFO_AGENT_WORDS):
                v = _value(e, k, t)
                word = np.float32(v).view(np.int32) if INFO_MM[k][1] else np.int32(v)
                info[t, e, INFO_WORLD_WORDS + k] = int(word)
    return rew, info, done


def _expected(e):
    """all 106 words of env e's only agent, written out"""
    w = [0.0] * 106
    if e == 0:
        w[0:8] = [4.0,              # steps
                  1.0,              # episodes
                  2.25, 2.0,        # the running episode: 2.0 + 0.25 over 2 steps (reset after step 1)
                  1.0, 1.0,         # completed episodes' reward sums: 1.5 - 0.5, squared
                  2.0, 4.0]         # their lengths: 2, squared
        w[8:10] = [3.25, 6.5625]    # reward: 1.5 - 0.5 + 2 + 0.25; 2.25 + 0.25 + 4 + 0.0625
    else:
        w[0:8] = [4.0, 0.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]
        w[8:10] = [3.0, 10.5]       # 0.5 + 0.5 - 1 + 3; 0.25 + 0.25 + 1 + 9
    for k in range(24):
        b = _c(k) + 8 * e           # the word's value at step 0; steps 1..3 add 1 each
        w[10 + 2 * k] = 4 * b + 6
        w[11 + 2 * k] = b * b + (b + 1) ** 2 + (b + 2) ** 2 + (b + 3) ** 2
        if e == 0:                  # the episode's last step is step 1
            w[58 + 2 * k] = b + 1
            w[59 + 2 * k] = (b + 1) ** 2
    return w


def test_reduce_steps_hand_written():
    rew, info, done = _example()
    st = EV.reduce_steps(rew, info, done, LAYOUT)
    assert st.dtype == torch.float64 and tuple(st.shape) == (E, 1, 106)
    for e in range(E):
        got, want = st[e, 0].tolist(), _expected(e)
        for i in range(106):
            assert got[i] == want[i], f"env {e} word {i}: {got[i]} != {want[i]}"
    # the per-type list form and the flattened info record give the same tensor
    assert torch.equal(EV.reduce_steps([rew], info.reshape(T * E, -1), done, LAYOUT), st)


def test_reduce_steps_int_and_float_words_are_widened_exactly():
    """an int32 word above 2^24 and a float32 word with a full mantissa keep every bit"""
    rew, info, done = _example()
    k_int = [k for k in range(24) if not INFO_MM[k][1]][0]
    k_f = [k for k in range(24) if INFO_MM[k][1]][0]
    big, f = 2 ** 31 - 1, np.float32(1.0000001)
    info[:, :, INFO_WORLD_WORDS + k_int] = big
    info[:, :, INFO_WORLD_WORDS + k_f] = int(f.view(np.int32))
    st = EV.reduce_steps(rew, info, done, LAYOUT)
    assert st[1, 0, 10 + 2 * k_int].item() == 4.0 * big
    assert st[1, 0, 11 + 2 * k_int].item() == 4.0 * (float(big) * float(big))
    assert st[1, 0, 10 + 2 * k_f].item() == 4.0 * float(f)
    assert st[1, 0, 11 + 2 * k_f].item() == 4.0 * (float(f) * float(f))


def test_eval_stats_against_numpy():
    rew, info, done = _example()
    ev = EV.EvalStats(EV.reduce_steps(rew, info, done, LAYOUT), LAYOUT)
    assert ev.n_types == 1 and ev.fields(0) == [n for n, _ in INFO_MM]
    assert ev.fields(0)[1] == "reward_portfolio_value" and ev.fields(0)[3] == "end_of_ep_pv"
    assert ev.steps(0) == 8 and ev.episodes(0) == 1 and ev.total_dones() == 1
    r = np.array(REWARDS, np.float64).ravel()
    assert ev.reward(0)["mean"] == r.mean() and math.isclose(ev.reward(0)["std"], r.std(), rel_tol=1e-12)
    per_step, at_end = ev.info(0), ev.info_at_episode_end(0)
    for k, (name, _) in enumerate(INFO_MM):
        v = np.array([_value(e, k, t) for e in range(E) for t in range(T)], np.float64)
        assert math.isclose(per_step[name]["mean"], v.mean(), rel_tol=1e-12), name
        assert math.isclose(per_step[name]["std"], v.std(), rel_tol=1e-12), name
        assert at_end[name] == {"mean": _value(0, k, 1), "std": 0.0}, name
    assert ev.episode_reward(0) == {"mean": 1.0, "std": 0.0}
    assert ev.episode_length(0) == {"mean": 2.0, "std": 0.0}
    s = ev.summary()
    assert s["total_dones"] == 1 and s["types"][0]["avg_reward"] == r.mean() and s["types"][0]["episodes"] == 1
    assert set(s["types"][0]["info"]) == set(ev.fields(0))


def test_eval_stats_zero_count_is_nan():
    rew, info, done = _example()
    st = EV.reduce_steps(rew, info, done, LAYOUT)[1:]          # env 1 alone: no episode completed
    ev = EV.EvalStats(st, LAYOUT)
    assert ev.episodes(0) == 0 and ev.steps(0) == 4
    assert math.isnan(ev.episode_reward(0)["mean"]) and math.isnan(ev.episode_reward(0)["std"])
    assert math.isnan(ev.episode_length(0)["std"])
    assert all(math.isnan(v["mean"]) and math.isnan(v["std"]) for v in ev.info_at_episode_end(0).values())
    empty = EV.EvalStats(torch.zeros((2, 1, 106), dtype=torch.float64), LAYOUT)
    assert math.isnan(empty.reward(0)["mean"]) and math.isnan(empty.reward(0)["std"])


def test_chunked_reduction_is_bit_identical():
    """[0:2] then [2:4] with the stats carried over == one call, on the example and on values whose
    sums round (random float32 rewards and info words, an episode end in each half)"""
    g = torch.Generator().manual_seed(5)
    rew_r = torch.randn((T, E, 1), generator=g, dtype=torch.float32) * 1e3
    info_r = torch.randn((T, E, LAYOUT.info_words), generator=g, dtype=torch.float32).view(torch.int32).clone()
    for k, (_, isf) in enumerate(INFO_MM):
        if not isf:
            info_r[:, :, INFO_WORLD_WORDS + k] = torch.randint(-2 ** 31, 2 ** 31 - 1, (T, E), generator=g,
                                                               dtype=torch.int64).to(torch.int32)
    done_r = torch.tensor([[False, True], [True, False], [False, False], [True, True]])
    for rew, info, done in (_example(), (rew_r, info_r, done_r)):
        whole = EV.reduce_steps(rew, info, done, LAYOUT)
        half = EV.reduce_steps(rew[:2], info[:2], done[:2], LAYOUT)
        keep = half.clone()
        both = EV.reduce_steps(rew[2:], info[2:], done[2:], LAYOUT, stats=half)
        assert torch.equal(half, keep), "the given stats tensor is not modified"
        assert torch.equal(both, whole)
        assert not torch.equal(half, whole)


def test_reduce_steps_refuses_bad_shapes():
    rew, info, done = _example()
    with pytest.raises(ValueError):
        EV.reduce_steps(rew.to(torch.float64), info, done, LAYOUT)
    with pytest.raises(ValueError):
        EV.reduce_steps(rew, info[:, :, :-1], done, LAYOUT)
    with pytest.raises(ValueError):
        EV.reduce_steps(rew, info, done[:3], LAYOUT)
    with pytest.raises(ValueError):
        EV.reduce_steps(rew, info, done, LAYOUT, stats=torch.zeros((E, 1, 105), dtype=torch.float64))


def test_several_actions_per_type_not_implemented():
    """the reference's FIXED_ACTIONS may list several actions for a type (drawn uniformly per step by
    JAX's categorical): refused by name, before any device work"""
    env = types.SimpleNamespace(multi_agent_config=types.SimpleNamespace(number_of_agents_per_type=[1, 1]),
                                action_widths=[1, 1], device="cpu")
    with pytest.raises(NotImplementedError, match="one action per agent type"):
        EV.evaluate_fixed_actions(env, [[1, 2], [0]], 8, 20, 0)
    with pytest.raises(NotImplementedError):
        EV.fixed_action_row(env, [4, [0, 1, 2]])
    assert EV.fixed_action_row(env, [[4], 2]).tolist() == [4, 2]      # the reference's [[4], [2]] and plain ints
    with pytest.raises(ValueError):
        EV.fixed_action_row(env, [4])
