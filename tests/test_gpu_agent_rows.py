"""The step's agent message rows ([cancels C][actions A]) of the 100/100 kernel without the rows
alias, which builds, filters and permutes them in registers (lane r = row r, hftlob.hip RegRows /
filter_regs), against the CPU oracle: every step's combined messages and state, bit for bit.

Message parity: 16 envs, 30 steps from the reset state of generate_day(n_msgs=20_000, seed=8),
reset keys arange(2E).reshape(E, 2) + 3, step k's keys the reset keys + 7k, through env.step,
through env.rollout (the same keys and actions in one launch) and through the persistent
rollout_sampled launch (its own key chain and sampled actions, replayed on the oracle).  The cases
must exercise _filter_messages: from the oracle's messages and the pre-step books each case counts
(a) the cancel rows that name a live order and (b) those the filter netted (quantity below the
resting order's), and asserts the floors measured on the oracle with these inputs:
  2_player_fq_fqc random actions 846 / 120, 3_player_fq_fqc_dir 827 / 123, agents [2, 2]
  1,676 / 262, every agent repeating action 0: 778 / 764.

Cancel slots: a record edited so that one agent rests more orders on a side than it has cancel
slots, at book slots 63, 64 and 99 (both 64-slot register sets and the last slot), and one with
exactly as many orders as slots; one env.step against the oracle over the same record.

The row-count rule (CPU): the register path holds the rows in the 64 lanes of message chunk 0, so
the launch code gives the 100/100 non-alias kernel to no config above 64 rows."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.layout import pack_env_cfg

E, T = 16, 30
_REF = {}


def _cfg(name, agents, shuffle):
    """the config with the MM type on the messages observation and raw observations saved: the
    step's combined message rows come back as info["agents"][0]["obs_raw"] (never blanked)"""
    from test_gpu_env import variant
    cfg = variant(builtin_config(name), "MarketMaking", observation_space="messages")
    w = dataclasses.replace(cfg.world_config, save_raw_observations=True, shuffle_action_messages=shuffle)
    cfg = dataclasses.replace(cfg, world_config=w)
    return dataclasses.replace(cfg, number_of_agents_per_type=list(agents)) if agents else cfg


def _launch_info(cfg):
    c, _ = pack_env_cfg(cfg, 4, 1000, True)
    info = _lib.LaunchInfo()
    rc = _lib.lib().hftlob_env_launch_info(C.byref(c), C.byref(info))
    return rc, c, info


def _largest_reg_agents():
    """the agent counts [mm, exe] of 2_player_fq_fqc with the most rows (then the most agents) that
    still launch the 100/100 kernel without the rows alias"""
    best = None
    for mm in range(1, 9):
        for exe in range(1, 9):
            rc, c, info = _launch_info(_cfg("2_player_fq_fqc", [mm, exe], True))
            if rc == 0 and (info.nfix, info.rows_alias) == (100, 0):
                k = (c.n_cancel_msgs + c.n_action_msgs, mm + exe)
                if best is None or k > best[0]:
                    best = (k, [mm, exe])
    return best[1]


CASES = {
    "2p": ("2_player_fq_fqc", None, False),
    "3p": ("3_player_fq_fqc_dir", None, False),
    "2p_22": ("2_player_fq_fqc", [2, 2], False),
    "2p_largest": ("2_player_fq_fqc", "largest", False),
    "2p_action0": ("2_player_fq_fqc", None, True),
}
FLOORS = {"2p": (400, 60), "3p": (400, 60), "2p_22": (400, 60), "2p_action0": (0, 380)}


def _day(w):
    key = ("day", w.n_data_msg_per_step * w.start_resolution)
    if key not in _REF:
        _REF[key] = generate_day(n_msgs=20_000, seed=8, snap_every=key[1])
    return _REF[key]


def _filter_counts(env, prev, msgs):
    """(a) cancel rows naming a live order of the pre-step books, (b) those with less than the
    resting order's quantity (the filter netted them against an action row)"""
    L, Cn = env.layout, env.layout.n_cancel_msgs
    nO = L.n_orders
    a = b = 0
    for e in range(prev.shape[0]):
        sides = {-1: prev[e, L.off_asks:L.off_asks + 6 * nO].reshape(nO, 6),
                 1: prev[e, L.off_bids:L.off_bids + 6 * nO].reshape(nO, 6)}
        for r in range(Cn):
            typ, side, q, p, oid, tid = msgs[e, r, :6]
            if typ != 2 or tid == 0:
                continue
            s = sides[int(side)]
            hit = np.nonzero((s[:, 2] == oid) & (s[:, 3] == tid) & (s[:, 0] == p))[0]
            if hit.size:
                a += 1
                b += int(q < s[hit[0], 1])
    return a, b


def _reference(case, shuffle):
    """The case's env, inputs and the oracle's per-step states and messages (computed once, shared
    by the three paths, never modified)."""
    from hftlob.env import MARLEnv
    from oracle import pyoracle as O
    key = (case, shuffle)
    if key in _REF:
        return _REF[key]
    name, agents, action0 = CASES[case]
    cfg = _cfg(name, _largest_reg_agents() if agents == "largest" else agents, shuffle)
    day = _day(cfg.world_config)
    env = MARLEnv(None, cfg, data=day)
    info = env.launch_info()
    assert (info["nfix"], info["rows_alias"]) == (100, 0), info
    k0 = (np.arange(2 * E, dtype=np.uint32).reshape(E, 2) + 3)
    keys = np.stack([k0 + np.uint32(7 * k) for k in range(T)])                 # [T, E, 2]
    acts = np.stack([np.zeros((E, env.action_words), np.int32) if action0 else O.sample_actions(env.cfg_c, keys[k])
                     for k in range(T)])
    init = env._init_states.cpu().numpy()
    st, _ = O.env_reset(env.cfg_c, k0, init)
    start = st.copy()
    states, msgs, a, b = [], [], 0, 0
    for k in range(T):
        res = O.env_step(env.cfg_c, keys[k], acts[k], day.msgs, init, st, extras=True)
        ak, bk = _filter_counts(env, st, res[7])
        a, b = a + ak, b + bk
        st = res[0]
        states.append(st.copy())
        msgs.append(res[7].copy())
    print(f"{case} shuffle={shuffle}: rows {env.layout.n_cancel_msgs}+{env.layout.n_action_msgs}, "
          f"cancel rows naming a live order {a}, netted by the filter {b}")
    if case in FLOORS:
        assert a >= FLOORS[case][0] and b >= FLOORS[case][1], (case, a, b)
    _REF[key] = dict(env=env, day=day, k0=k0, keys=keys, acts=acts, init=init, start=start, states=states, msgs=msgs)
    return _REF[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def _raw_msgs(info):
    return info["agents"][0]["obs_raw"].cpu().numpy()


def _same(tag, want, got):
    bad = np.argwhere(want != got)
    assert bad.size == 0, f"{tag}: differs at {bad[:5].tolist()} oracle {want[tuple(bad[0])]} gpu {got[tuple(bad[0])]}"


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "noshuffle"])
@pytest.mark.parametrize("case", list(CASES))
def test_message_parity_step(case, shuffle):
    R = _reference(case, shuffle)
    env = R["env"]
    params = env.default_params
    _, state = env.reset(_dev(R["k0"]), params)
    _same("reset", R["start"], state.buf.cpu().numpy())
    for k in range(T):
        _, state, _, _, info = env.step(_dev(R["keys"][k]), state, _dev(R["acts"][k]), params)
        m = _raw_msgs(info)                                                # [E, n, M, 8]: every agent sees the same rows
        _same(f"step {k}: msgs", np.broadcast_to(R["msgs"][k][:, None], m.shape), m)
        _same(f"step {k}: state", R["states"][k], state.buf.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "noshuffle"])
@pytest.mark.parametrize("case", list(CASES))
def test_message_parity_rollout_actions(case, shuffle):
    R = _reference(case, shuffle)
    env = R["env"]
    params = env.default_params
    _, state = env.reset(_dev(R["k0"]), params)
    _, state, _, _, info = env.rollout(_dev(R["keys"]), state, _dev(R["acts"]), params, per_step=True)
    m = _raw_msgs(info)
    M = env.layout.n_msgs
    m = m.reshape(T, E, -1, M, 8)
    for k in range(T):
        _same(f"step {k}: msgs", np.broadcast_to(R["msgs"][k][:, None], m[k].shape), m[k])
    _same("end state", R["states"][-1], state.buf.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "noshuffle"])
@pytest.mark.parametrize("case", [c for c in CASES if not CASES[c][2]])
def test_message_parity_rollout_sampled(case, shuffle):
    """the persistent sampled launch draws its own keys and actions: replayed on the oracle"""
    from oracle import pyoracle as O
    R = _reference(case, shuffle)
    env = R["env"]
    params = env.default_params
    _, state = env.reset(_dev(R["k0"]), params)
    master = np.array([0, 7], np.uint32)
    k_in = _dev(master)
    k_out = torch.empty_like(k_in)
    _, state, _, _, info = env.rollout_sampled(k_in, k_out, state, params, T, per_step=True, n_slices=0)
    M = env.layout.n_msgs
    m = _raw_msgs(info).reshape(T, E, -1, M, 8)
    st = R["start"]
    for k in range(T):
        ks = O.split_keys(master[None], E + 1)[0]
        master, sk = ks[0].copy(), ks[1:].copy()
        res = O.env_step(env.cfg_c, sk, O.sample_actions(env.cfg_c, sk), R["day"].msgs, R["init"], st, extras=True)
        st = res[0]
        _same(f"step {k}: msgs", np.broadcast_to(res[7][:, None], m[k].shape), m[k])
    _same("end state", st, state.buf.cpu().numpy())
    _same("carried key", master, k_out.cpu().numpy().view(np.uint32))


def _write_orders(rec, L, side_off, slots, tid, oid0, p0, dp, t):
    nO = L.n_orders
    tab = rec[side_off:side_off + 6 * nO].reshape(nO, 6)
    for j, s in enumerate(slots):
        tab[s] = (p0 + dp * (j + 1), 10 + j, oid0 + s, tid, t[0], t[1])


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["more_than_slots", "exactly_slots"])
def test_cancel_slots_across_register_sets(exact):
    """Even envs: the MM agent (1 cancel slot a side) rests orders at slots 63, 64, 99 of both sides
    (or one, at slot 99 / 64); odd envs: the EXE agent (4 slots on its task's side) at slots 2, 5,
    63, 64, 99 of both sides (or at 5, 63, 64, 99).  One env.step vs the oracle on the same record."""
    from hftlob.env import MARLEnv
    from oracle import pyoracle as O
    R = _reference("2p", True)
    env, day, init = R["env"], R["day"], R["init"]
    L, c = env.layout, env.cfg_c
    params = env.default_params
    rec = R["states"][4].copy()                                   # books a few steps in
    tid_mm, tid_exe = c.types[0].trader_id0, c.types[1].trader_id0
    nO = L.n_orders
    assert nO == 100
    for e in range(E):
        r = rec[e]
        asks = r[L.off_asks:L.off_asks + 6 * nO].reshape(nO, 6)
        bids = r[L.off_bids:L.off_bids + 6 * nO].reshape(nO, 6)
        for tab in (asks, bids):                                  # the agents' own resting orders go first
            tab[(tab[:, 3] == tid_mm) | (tab[:, 3] == tid_exe)] = -1
        ba, bb = asks[asks[:, 0] > 0, 0].min(), bids[bids[:, 0] > 0, 0].max()
        t = (int(r[L.off_world]), int(r[L.off_world + 1]))
        if e % 2 == 0:
            tid, n_slots = tid_mm, 1
            s_b, s_a = ([99], [64]) if exact else ([63, 64, 99], [63, 64, 99])
        else:
            tid, n_slots = tid_exe, 4
            s_b = s_a = [5, 63, 64, 99] if exact else [2, 5, 63, 64, 99]
        _write_orders(r, L, L.off_bids, s_b, tid, 7_000_000, bb, -100, t)
        _write_orders(r, L, L.off_asks, s_a, tid, 8_000_000, ba, 100, t)
        for tab, slots in ((bids, s_b), (asks, s_a)):             # the record really holds those rows
            held = np.nonzero(tab[:, 3] == tid)[0].tolist()
            assert held == slots and (len(held) == n_slots if exact else len(held) > n_slots), (e, held)
    keys = R["keys"][5]
    acts = R["acts"][5]
    res = O.env_step(c, keys, acts, day.msgs, init, rec, extras=True)
    a, _ = _filter_counts(env, rec, res[7])
    assert a >= E, "every env's agent cancels at least one of the written orders"
    _, state = env.reset(_dev(R["k0"]), params)
    state.buf.copy_(torch.from_numpy(rec).cuda())
    _, state, _, _, info = env.step(_dev(keys), state, _dev(acts), params)
    m = _raw_msgs(info)
    _same("msgs", np.broadcast_to(res[7][:, None], m.shape), m)
    _same("state", res[0], state.buf.cpu().numpy())


def test_reg_rows_need_at_most_64_rows():
    """hftlob_env_launch_info over agent counts of two 100/100 configs: a config that launches the
    100/100 kernel without the rows alias (the register path) has at most 64 agent rows; with more
    rows it takes the rows alias or a general-size kernel (nfix 0), never (100, 0).  Today the LDS
    share rule alone sends every such config to the alias; the launch code states the bound itself
    (reg_rows_ok), so a change of sizes cannot launch the register path past its lanes."""
    if not __import__("os").path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built")
    seen_reg = seen_more = 0
    for name in ("2_player_fq_fqc", "default"):
        for mm in range(1, 17):
            for exe in range(1, 17):
                if mm + exe > 32:
                    continue
                cfg = dataclasses.replace(builtin_config(name), number_of_agents_per_type=[mm, exe])
                rc, c, info = _launch_info(cfg)
                rows = c.n_cancel_msgs + c.n_action_msgs
                if rc != 0:
                    assert rows > 128, (name, mm, exe, rows)      # (MAX_AGENT_ROWS: check_env refuses)
                    continue
                if (info.nfix, info.rows_alias) == (100, 0):
                    seen_reg += 1
                    assert rows <= 64, (name, mm, exe, rows)
                if rows > 64:
                    seen_more += 1
                    assert info.rows_alias == 1 or info.nfix == 0, (name, mm, exe, rows)
                    assert info.slot_sets == 2
    assert seen_reg and seen_more
    rc, c, info = _launch_info(builtin_config("2_player_fq_fqc"))
    assert (rc, info.slot_sets, info.nfix, info.rows_alias) == (0, 2, 100, 0)
