"""The per-episode records on the CPU: hftlob.evaluate.reduce_steps(max_episodes=) against a plain numpy
float64 loop on a hand-made example, the index rule (word 1 before the step's increment, the cap, a
carried start), EpisodeLog on a hand-written tensor, the files EpisodeLog.save / save_combinations write
read back with pandas / json / numpy, and the three entry points' declarations.

The example: T = 6 steps, E = 4 envs, A = 2 agents (a market maker and an execution agent, so the two
float-word masks differ).  Env 0 never ends an episode, env 1 ends one at t = 0, env 2 ends three
(t = 1, 2 and T - 1), env 3 one at t = T - 1.  One float word of the market maker is NaN at an episode
end."""
import json
import math
import os
import re
import types

import numpy as np
import pandas as pd
import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.layout import AGENT_EXE, AGENT_MM, INFO_AGENT_WORDS, INFO_EXE, INFO_MM, INFO_WORLD_WORDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, E, A = 6, 4, 2
W = _lib.EPISODE_WORDS
LAYOUT = types.SimpleNamespace(agent_kinds=[AGENT_MM, AGENT_EXE], agent_types=[0, 1],
                               info_words=INFO_WORLD_WORDS + A * INFO_AGENT_WORDS)
ENDS = {0: [], 1: [0], 2: [1, 2, T - 1], 3: [T - 1]}
NAN_AT = (2, 2, 0, 3)      # (t, env, agent, word): a float32 word of INFO_MM
assert INFO_MM[NAN_AT[3]][1]


def _is_float(a, k):
    fields = INFO_MM if LAYOUT.agent_kinds[a] == AGENT_MM else INFO_EXE
    return k < len(fields) and bool(fields[k][1])


def _example(seed=3):
    """float32 rewards [T, E, A], int32 info [T, E, info_words], bool dones [T, E]: inexact float sums,
    int words past 2^24 (so a float widening would differ from the int one)"""
    g = np.random.default_rng(seed)
    rew = g.normal(size=(T, E, A)).astype(np.float32)
    info = g.integers(-2 ** 30, 2 ** 30, size=(T, E, LAYOUT.info_words)).astype(np.int32)
    for a in range(A):
        for k in range(INFO_AGENT_WORDS):
            if _is_float(a, k):
                col = INFO_WORLD_WORDS + a * INFO_AGENT_WORDS + k
                info[:, :, col] = g.normal(scale=100.0, size=(T, E)).astype(np.float32).view(np.int32)
    t, e, a, k = NAN_AT
    info[t, e, INFO_WORLD_WORDS + a * INFO_AGENT_WORDS + k] = np.float32(np.nan).view(np.int32)
    done = np.zeros((T, E), dtype=bool)
    for e, ts in ENDS.items():
        done[ts, e] = True
    return torch.from_numpy(rew), torch.from_numpy(info), torch.from_numpy(done)


def _numpy_records(rew, info, done, cap, first=None, episodes=None):
    """the records as a plain float64 loop: `first` [E] is each env's episode count before the steps"""
    rew, info, done = rew.numpy(), info.numpy(), done.numpy()
    nT = rew.shape[0]
    out = np.zeros((E, A, cap, W)) if episodes is None else episodes.copy()
    for e in range(E):
        for a in range(A):
            i = 0 if first is None else int(first[e])
            run, length = 0.0, 0.0
            for t in range(nT):
                run += float(rew[t, e, a])
                length += 1.0
                if done[t, e]:
                    if i < cap:
                        out[e, a, i, 0], out[e, a, i, 1] = run, length
                        for k in range(INFO_AGENT_WORDS):
                            w = info[t, e, INFO_WORLD_WORDS + a * INFO_AGENT_WORDS + k]
                            out[e, a, i, 2 + k] = float(w.view(np.float32)) if _is_float(a, k) else float(w)
                    i += 1
                    run, length = 0.0, 0.0
    return out


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    got = got.numpy()
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def test_reduce_steps_records_against_numpy():
    rew, info, done = _example()
    stats, ep = EV.reduce_steps(rew, info, done, LAYOUT, max_episodes=4)
    assert ep.dtype == torch.float64 and tuple(ep.shape) == (E, A, 4, W)
    assert _same(ep, _numpy_records(rew, info, done, 4))
    assert stats[:, 0, 1].tolist() == [0.0, 1.0, 3.0, 1.0]
    assert bool((ep[0] == 0).all()) and bool((ep[2, :, 3] == 0).all()), "slots past the count stay as they were"
    assert ep[1, 0, 0, 1] == 1.0 and ep[3, 1, 0, 1] == T, "an end at t = 0 and at t = T - 1"
    assert ep[2, :, :3, 1].tolist() == [[2.0, 1.0, 3.0]] * 2
    t, e, a, k = NAN_AT
    assert math.isnan(ep[e, a, 1, 2 + k]) and not bool(ep[e, 1].isnan().any())
    # the records are what the accumulators add: their sums are words 4, 6 and 58 + 2k
    assert torch.equal(ep[3, :, 0, 0], stats[3, :, 4]) and torch.equal(ep[3, :, 0, 2:], stats[3, :, 58::2])


def test_without_max_episodes_the_result_is_the_stats_tensor():
    rew, info, done = _example()
    st = EV.reduce_steps(rew, info, done, LAYOUT)
    assert isinstance(st, torch.Tensor) and tuple(st.shape) == (E, A, _lib.EVAL_WORDS)
    both = EV.reduce_steps(rew, info, done, LAYOUT, max_episodes=2)
    assert isinstance(both, tuple) and len(both) == 2
    assert bool(((both[0] == st) | (both[0].isnan() & st.isnan())).all())


def test_a_run_cut_in_two_equals_one_call():
    rew, info, done = _example()
    whole = EV.reduce_steps(rew, info, done, LAYOUT, max_episodes=3)
    st, ep = EV.reduce_steps(rew[:2], info[:2], done[:2], LAYOUT, max_episodes=3)
    keep = ep.clone()
    st2, ep2 = EV.reduce_steps(rew[2:], info[2:], done[2:], LAYOUT, stats=st, episodes=ep)
    assert torch.equal(ep, keep), "a given episodes tensor is cloned"
    assert _same(ep2, whole[1].numpy()) and _same(st2, whole[0].numpy())
    assert ep2[2, 0, 1, 1] == 1.0 and ep2[2, 0, 2, 1] == 3.0


def test_a_start_from_word_1_of_5_writes_at_index_5():
    rew, info, done = _example()
    st0 = torch.zeros((E, A, _lib.EVAL_WORDS), dtype=torch.float64)
    st0[:, :, 1] = 5.0
    sentinel = torch.full((E, A, 8, W), -7.0, dtype=torch.float64)
    st, ep = EV.reduce_steps(rew, info, done, LAYOUT, stats=st0, episodes=sentinel)
    want = _numpy_records(rew, info, done, 8, first=[5] * E, episodes=sentinel.numpy())
    assert _same(ep, want)
    assert bool((ep[:, :, :5] == -7.0).all()) and ep[1, 0, 5, 1] == 1.0 and bool((ep[1, :, 6:] == -7.0).all())
    assert ep[2, 1, 7, 1] == 3.0 and st[2, 0, 1] == 8.0


def test_cap_of_one_keeps_the_first_and_reports_dropped():
    rew, info, done = _example()
    st, ep = EV.reduce_steps(rew, info, done, LAYOUT, max_episodes=1)
    assert _same(ep, _numpy_records(rew, info, done, 1))
    assert ep[2, 0, 0, 1] == 2.0, "env 2's first episode (2 steps), not a later one"
    log = EV.EpisodeLog(ep, st, LAYOUT)
    assert log.count.tolist() == [0, 1, 1, 1] and log.dropped == 2 and len(log) == 3
    assert st[2, 0, 1] == 3.0 > log.cap, "overflow shows as word 1 > cap"


def test_bad_cap_is_named():
    rew, info, done = _example()
    for cap in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="ep_cap"):
            EV.reduce_steps(rew, info, done, LAYOUT, max_episodes=cap)
    with pytest.raises(ValueError, match="episodes must be"):
        EV.reduce_steps(rew, info, done, LAYOUT, episodes=torch.zeros((E, A, 2, W - 1), dtype=torch.float64))


def _hand_log():
    """2 envs, cap 3: env 0 completed 2 episodes, env 1 completed 4 (one dropped)"""
    ep = torch.zeros((2, A, 3, W), dtype=torch.float64)
    st = torch.zeros((2, A, _lib.EVAL_WORDS), dtype=torch.float64)
    st[0, :, 1], st[1, :, 1] = 2.0, 4.0
    mm = [[1.0, -3.0, 99.0], [4.0, 0.0, 2.0]]          # agent 0's episode rewards (99: a stale slot past the count)
    ex = [[10.0, 20.0, 99.0], [30.0, 40.0, 50.0]]
    for e in range(2):
        for i in range(3):
            ep[e, 0, i, 0], ep[e, 1, i, 0] = mm[e][i], ex[e][i]
            ep[e, :, i, 1] = 65.0 + i
            ep[e, 1, i, 2 + [n for n, _ in INFO_EXE].index("drift")] = 0.5 * (3 * e + i)
    return EV.EpisodeLog(ep, st, LAYOUT)


def test_episode_log_by_hand():
    log = _hand_log()
    assert log.count.tolist() == [2, 3] and log.dropped == 1 and len(log) == 5 and log.cap == 3
    # rows: (env 0, 0), (env 0, 1), (env 1, 0), (env 1, 1), (env 1, 2)
    assert log.rewards().tolist() == [[1.0, 10.0], [-3.0, 20.0], [4.0, 30.0], [0.0, 40.0], [2.0, 50.0]]
    assert log.env.tolist() == [0, 0, 1, 1, 1]
    assert log.lengths().tolist() == [65.0, 66.0, 65.0, 66.0, 67.0]
    assert log.field(1, "drift").tolist() == [[0.0], [0.5], [1.5], [2.0], [2.5]]
    with pytest.raises(ValueError, match="no info field"):
        log.field(0, "drift")
    # the market maker's rewards sorted: -3, 0, 1, 2, 4
    assert log.quantiles(0, [0.0, 0.5, 0.75, 1.0]).tolist() == [-3.0, 1.0, 2.0, 4.0]
    assert log.quantiles(0, [0.125]).tolist() == [-1.5]                 # halfway between -3 and 0
    assert log.cvar(0, 0.4) == -1.5                                     # the 2 worst of 5: (-3 + 0) / 2
    assert log.cvar(0, 0.2) == -3.0 and log.cvar(0, 1.0) == 0.8
    assert log.cvar(1, 0.5, what="drift") == (0.0 + 0.5 + 1.5) / 3   # ceil(2.5) = 3 values
    counts, edges = log.histogram(0, bins=7)
    assert counts.tolist() == [1, 0, 0, 1, 1, 1, 1] and edges[0] == -3.0 and edges[-1] == 4.0
    s = log.summary()
    assert json.loads(json.dumps(s)) == s
    assert s["episodes"] == 5 and s["dropped"] == 1 and s["types"][1]["episode_reward"]["mean"] == 30.0
    assert s["types"][0]["episode_reward"]["quantiles"]["0.5"] == 1.0


def test_save_formats(tmp_path):
    log = _hand_log()
    want = log.rewards().numpy()
    logs = {"BB": log, "LL": log}
    p = str(tmp_path / "ep.csv")
    EV.save_combinations(p, logs)
    df = pd.read_csv(p)
    assert list(df.columns) == ["Configuration", "Episode", "MarketMaker", "ExecutionAgent"]
    assert sorted(df["Configuration"].unique()) == ["Config_BB", "Config_LL"]
    for name, group in df.groupby("Configuration"):
        group = group.sort_values("Episode")
        assert group["Episode"].tolist() == [0, 1, 2, 3, 4]
        assert (group[["MarketMaker", "ExecutionAgent"]].to_numpy() == want).all()
    p = str(tmp_path / "ep.json")
    EV.save_combinations(p, logs)
    data = json.load(open(p))
    assert sorted(data) == ["Config_BB", "Config_LL"] and (np.array(data["Config_LL"]) == want).all()
    p = str(tmp_path / "ep.npz")
    EV.save_combinations(p, logs)
    assert os.listdir(tmp_path).count("ep.npz") == 1 and not os.path.exists(p + ".npz")
    z = np.load(p)
    assert sorted(z.files) == ["Config_BB", "Config_LL"]
    assert z["Config_BB"].dtype == np.float64 and (z["Config_BB"] == want).all()
    p = str(tmp_path / "one.npz")
    log.save(p)
    assert np.load(p).files == ["Config"]
    log.save(str(tmp_path / "one.csv"), name="Config_BL")
    assert pd.read_csv(tmp_path / "one.csv")["Configuration"].tolist() == ["Config_BL"] * 5
    with pytest.raises(ValueError, match="suffix"):
        log.save(str(tmp_path / "ep.txt"))
    # three agents: Agent_i columns
    lay3 = types.SimpleNamespace(agent_kinds=[AGENT_MM, AGENT_EXE, AGENT_EXE], agent_types=[0, 1, 2],
                                 info_words=INFO_WORLD_WORDS + 3 * INFO_AGENT_WORDS)
    st = torch.zeros((1, 3, _lib.EVAL_WORDS), dtype=torch.float64)
    st[:, :, 1] = 1.0
    EV.EpisodeLog(torch.ones((1, 3, 2, W), dtype=torch.float64), st, lay3).save(str(tmp_path / "three.csv"))
    assert list(pd.read_csv(tmp_path / "three.csv").columns) == ["Configuration", "Episode", "Agent_0", "Agent_1",
                                                                 "Agent_2"]


def test_symbols_and_record_size():
    header = open(os.path.join(ROOT, "include", "hftlob.h")).read()
    assert re.search(r"#define\s+HFTLOB_EPISODE_WORDS\s+26\b", header) and _lib.EPISODE_WORDS == 26 == 2 + INFO_AGENT_WORDS
    for name in ("hftlob_env_rollout_eval_episodes", "hftlob_env_rollout_eval_drawn_episodes",
                 "hftlob_eval_tally_episodes"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert re.search(r"double\*\s+episodes\b[^,]*,\s*int\s+ep_cap\s*,\s*void\*\s+stream\s*$", m.group(1)), name
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        k = 64  # (never dereferenced: the refusals come first)
        assert L.hftlob_eval_tally_episodes(1, 1, 1, 64, k, k, k, (_lib.C.c_uint32 * 1)(0), k, None, 4, None) == -1
        assert L.hftlob_eval_tally_episodes(1, 1, 1, 64, k, k, k, (_lib.C.c_uint32 * 1)(0), k, k, 0, None) == -1
        assert b"ep_cap" in L.hftlob_last_error()
        assert L.hftlob_version() == 8
