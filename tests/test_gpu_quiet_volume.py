"""The lazy-volume mode of the persistent rollout's quiet steps (env_step_dev's LAZY, hftlob.hip).

A quiet step of a baked config's k_env_rollout keeps no volume at the best price: its rescans
compute the price alone, a level's exhaustion is found from the price column where a row is
cleared, and the emitting last step recomputes both quotes from the book.  The mode is decided at
compile time, so it runs exactly where the launch takes a baked instantiation (baked_id() >= 0);
every other launch (the switch off, a config with exclude_extreme_spreads, whose quiet steps store
the whole best-quote arrays) runs the eager handlers.  Every case compares a persistent
rollout_sampled launch (per_step = False, n_slices = 0) bit for bit with the same number of
step_sampled launches (k_env_step: every step emitting, the whole best-quote arrays stored) and with
the oracle's C rollout.  The references of a (config, envs, steps) case are computed once and shared
between the baked and the general run."""
import dataclasses

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import LobsterDay, generate_day

pytestmark = pytest.mark.gpu

BAKED = {"2_player_fq_fqc": 0, "3_player_fq_fqc_dir": 1}
MID, TICK = 2_000_000, 100
_ENVS, _REFS = {}, {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def _cfg(name):
    if name == "mm_excl":  # an MM type that excludes extreme spreads: store_best stays true in the resident loop
        cfg = builtin_config("2_player_fq_fqc")
        agents = dict(cfg.dict_of_agents_configs)
        agents["MarketMaking"] = dataclasses.replace(agents["MarketMaking"], exclude_extreme_spreads=True)
        return dataclasses.replace(cfg, dict_of_agents_configs=agents)
    return builtin_config(name)


# ----------------------------------------------------------------- the hand-made day
# One block of 64 steps x 100 data messages, repeated for every window of the day (the windows of
# the metric config tile the day: they start every 6400 messages and hold 6400), so every env
# replays the same block from its start whichever window its reset draws.  Message rows are
# [type, side, qty, price, trader id, order id, time s, time ns] (hftlob.data.synthetic).
P_ASK, P_BID = MID + 100, MID - 100          # a new best price inside the snapshot's spread
STEP_A, STEP_B, STEP_D = 1, 3, 5  # asks at the step, bids at the step after (D: two steps a side)
AT = 10                                      # a scenario's first data message of its step
T_HAND = 10                                  # steps 0..8 quiet (D's bid half ends at step 8), step 9 emits


def _hand_block():
    rows = [[] for _ in range(64)]
    oid = [20_000_000]

    def new():
        oid[0] += 1
        return oid[0]

    def add(t, side, p, q):
        o = new()
        rows[t].append((1, side, q, p, o, o))
        return o

    def cancel(t, side, p, q, o):
        rows[t].append((2, side, q, p, o, o))

    def fill(t, upto):  # cancels of ids no row holds (the replayed day's common message)
        while len(rows[t]) < upto:
            k = len(rows[t])
            side = 1 if k % 2 else -1
            o = new()
            rows[t].append((2, side, 1 + k % 3, MID - side * (500 + 100 * (k % 10)), o, o))

    def wipe(t, side):  # one crossing order empties the side; its remainder is cancelled
        far = MID - side * 100_000
        x = add(t, -side, far, 1_000_000)
        cancel(t, -side, far, 1_000_000, x)

    def refill(t, side):
        for k in range(10):
            add(t, side, MID - side * (500 + 100 * k), 50)

    for s, side, P in ((0, -1, P_ASK), (1, 1, P_BID)):
        back = MID - side * 1000              # the level behind the scenario's best level
        # A (and C: a side emptied and refilled): the agents' orders out of the way, a level at `back`, two
        # orders at the new best price P; cancel one (the level survives), then the other (`back` is best)
        t = STEP_A + s
        fill(t, AT)
        wipe(t, side)
        add(t, side, back, 50)
        o1, o2 = add(t, side, P, 10), add(t, side, P, 10)
        cancel(t, side, P, 10, o1)
        cancel(t, side, P, 10, o2)
        refill(t, side)
        # B: a crossing order that consumes two rows of the best level, one that leaves a partial row
        t = STEP_B + s
        fill(t, AT)
        wipe(t, side)
        add(t, side, back, 50)
        add(t, side, P, 10), add(t, side, P, 10)
        add(t, -side, P, 20)
        add(t, side, P, 10)
        o6 = add(t, side, P, 10)
        add(t, -side, P, 15)
        cancel(t, side, P, 5, o6)
        refill(t, side)
        # D: 105 orders behind the best fill the side's 100 rows, so that adds evict
        t = STEP_D + 2 * s
        fill(t, AT)
        for k in range(105):
            tt = t if len(rows[t]) < 100 else t + 1
            add(tt, side, MID - side * (2000 + 100 * k), 1)
    for t in range(64):
        fill(t, 100)
        assert len(rows[t]) == 100
    return np.array([r for t in range(64) for r in rows[t]], dtype=np.int64)


def _hand_day(n_windows=3):
    blk = _hand_block()
    n = len(blk) * n_windows
    msgs = np.zeros((n, 8), dtype=np.int64)
    msgs[:, :6] = np.tile(blk, (n_windows, 1))
    t_ns = (np.arange(n, dtype=np.int64) + 1) * 3_000_000          # 3 ms apart, from 09:30
    msgs[:, 6] = 34200 + t_ns // 1_000_000_000
    msgs[:, 7] = t_ns % 1_000_000_000
    book = np.zeros(40, dtype=np.int64)
    for k in range(10):
        book[4 * k:4 * k + 4] = (MID + 500 + 100 * k, 50, MID - 500 - 100 * k, 50)
    return LobsterDay(msgs=msgs.astype(np.int32), books=np.tile(book, (n_windows, 1)).astype(np.int32),
                      snap_idx=np.arange(n_windows) * len(blk), tick_size=TICK)


def _env(name, day_name):
    from hftlob.env import MARLEnv
    key = (name, day_name)
    if key not in _ENVS:
        cfg = _cfg(name)
        w = cfg.world_config
        day = _hand_day() if day_name == "hand" else generate_day(n_msgs=20_000, seed=8,
                                                                  snap_every=w.n_data_msg_per_step * w.start_resolution)
        _ENVS[key] = MARLEnv(None, cfg, data=day, return_info=True)
    return _ENVS[key]


def _outputs(obs, rew, dones, env):
    return ([x.clone() for x in obs], [x.clone() for x in rew], dones["__all__"].clone(),
            [x.clone() for x in dones["agents"]], env.last_info_words.clone())


def _reference(name, day_name, E, T):
    """T step_sampled launches from the reset state and the oracle's rollout over the same steps:
    (start state, end state, carried key, the last step's outputs, each step's state, oracle state, oracle key)"""
    key = (name, day_name, E, T)
    if key not in _REFS:
        from oracle import pyoracle as O
        env = _env(name, day_name)
        params = env.default_params
        _, s = env.reset(_dev(np.arange(2 * E, dtype=np.uint32).reshape(E, 2) + 3), params)
        start = s.buf.clone()
        kbuf = [_dev(np.array([0, 7], np.uint32)), torch.empty(2, dtype=torch.int32, device="cuda")]
        per_step = []
        for k in range(T):
            obs, s, rew, dones, _ = env.step_sampled(kbuf[k % 2], kbuf[(k + 1) % 2], s, params)
            per_step.append(s.buf.cpu().numpy().copy())
        out = _outputs(obs, rew, dones, env)
        o_st, o_key = O.rollout_sampled(env.cfg_c, np.array([0, 7], np.uint32), env.data.msgs,
                                        env._init_states.cpu().numpy(), start.cpu().numpy(), T)
        _REFS[key] = (start, s.buf.clone(), kbuf[T % 2].clone(), out, per_step, o_st, o_key)
    return _REFS[key]


def _rollout(name, day_name, E, T, baked, graph=False):
    """one persistent rollout_sampled launch of T steps from the reference's start state, with the
    switch hftlob_set_baked set to `baked`; asserts the launched instantiation and the parity"""
    env = _env(name, day_name)
    start, end, key_end, out, _, o_st, o_key = _reference(name, day_name, E, T)
    info = env.launch_info()
    assert (info["slot_sets"], info["nfix"], info["random_cancel"], info["rows_alias"]) == (2, 100, 0, 0), info
    params = env.default_params
    prev = _lib.set_baked(baked)
    try:
        want = BAKED.get(name, -1) if baked else -1
        assert env.baked_id() == want, "the instantiation the launch takes"
        _, s = env.reset(_dev(np.arange(2 * E, dtype=np.uint32).reshape(E, 2) + 3), params)
        assert (s.buf == start).all()
        k_in, k_out = _dev(np.array([0, 7], np.uint32)), torch.empty(2, dtype=torch.int32, device="cuda")
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up outside the capture
                env.rollout_sampled(k_in, k_out, s, params, T, per_step=False, n_slices=0)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                res = env.rollout_sampled(k_in, k_out, s, params, T, per_step=False, n_slices=0)
            s.buf.copy_(start)
            k_out.zero_()
            g.replay()
        else:
            res = env.rollout_sampled(k_in, k_out, s, params, T, per_step=False, n_slices=0)
        torch.cuda.synchronize()
    finally:
        _lib.set_baked(prev)
    obs, s, rew, dones, _ = res
    got = _outputs(obs, rew, dones, env)
    assert (k_out == key_end).all(), "carried key"
    bad = torch.nonzero(s.buf != end)
    assert bad.numel() == 0, f"end state (env, word) {bad[:5].tolist()}"
    # the whole best-quote arrays, volumes included, are part of that state: (price, volume) x M rows a side
    L, M = env.layout, env.layout.n_msgs
    for off in (L.off_best_asks, L.off_best_bids):
        a = s.buf[:, off:off + 2 * M].cpu().numpy().reshape(E, M, 2)
        assert (a == end[:, off:off + 2 * M].cpu().numpy().reshape(E, M, 2)).all()
        assert (a[:, :, 1] > 0).any(), "the arrays hold volumes"
    for i, (a, b) in enumerate(zip(got[:2], out[:2])):
        assert all((x == y).all() for x, y in zip(a, b)), f"last step {'obs' if i == 0 else 'rewards'}"
    assert (got[2] == out[2]).all() and all((x == y).all() for x, y in zip(got[3], out[3])), "last step dones"
    assert (got[4] == out[4]).all(), "last step info"
    g_st = s.buf.cpu().numpy()
    assert (g_st == o_st).all(), f"end state differs from the oracle at {np.argwhere(g_st != o_st)[:5].tolist()}"
    assert (k_out.cpu().numpy().view(np.uint32) == o_key).all(), "carried key differs from the oracle"
    return env, g_st


# 70 steps from the reset state: every env's episode end (64-step windows) and auto-reset fall inside the quiet loop
@pytest.mark.parametrize("name,E,baked", [("2_player_fq_fqc", 5, True), ("2_player_fq_fqc", 64, True),
                                           ("3_player_fq_fqc_dir", 5, True), ("2_player_fq_fqc", 5, False),
                                           ("2_player_fq_fqc", 64, False), ("3_player_fq_fqc_dir", 5, False),
                                           ("mm_excl", 5, True)])
def test_quiet_volume_parity(name, E, baked):
    """baked id 0 / 1 (the lazy-volume quiet steps), the same configs on the general 100/100 kernel, and
    a config whose quiet steps store the whole arrays (it equals no baked config: the eager handlers)"""
    env, st = _rollout(name, "gen", E, 70, baked)
    assert (st[:, env.layout.off_loaded + 5] < 70).all(), "every env crossed an episode end"


def _quotes(env, st, e):
    L, M = env.layout, env.layout.n_msgs
    a = st[e, L.off_best_asks:L.off_best_asks + 2 * M].reshape(M, 2)
    b = st[e, L.off_best_bids:L.off_best_bids + 2 * M].reshape(M, 2)
    return a, b


@pytest.mark.parametrize("T", [T_HAND, STEP_B + 1])
def test_quiet_volume_level_exhaustion(T):
    """the hand-made day (above) at 2 envs: a side emptied and refilled, best levels emptied by cancels
    and by crossing orders, a side filled until adds evict, all in quiet steps of the baked kernel;
    T = 10: the emitting step follows them, T = 4: it is the step of the crossing orders on the ask
    side.  The per-step reference's whole arrays show that the scenarios took place."""
    E = 2
    env, _ = _rollout("2_player_fq_fqc", "hand", E, T, True)
    if T != T_HAND:
        return
    per_step = _reference("2_player_fq_fqc", "hand", E, T)[4]
    r0 = env.layout.n_msgs - 100 + AT  # the record row of a scenario's first data message
    for e in range(E):
        for s, P in ((0, P_ASK), (1, P_BID)):
            back = [MID + (1000 if s == 0 else -1000), 50]
            # A: the side empty (a -1 quote is recorded with volume 0) twice, `back`, then P with 10, 20, 10, `back`
            q = _quotes(env, per_step[STEP_A + s], e)[s][r0:r0 + 8]
            print("A", e, s, q.tolist())
            assert q[0, 1] == 0 and q[1, 1] == 0
            assert q[2:7].tolist() == [back, [P, 10], [P, 20], [P, 10], back]
            assert q[7].tolist() == [MID + (500 if s == 0 else -500), 50]
            # B: two rows consumed at once; then a partial row of 5, cancelled
            q = _quotes(env, per_step[STEP_B + s], e)[s][r0:r0 + 10]
            print("B", e, s, q.tolist())
            assert q[0, 1] == 0 and q[1, 1] == 0
            assert q[2:10].tolist() == [back, [P, 10], [P, 20], back, [P, 10], [P, 20], [P, 5], back]
        L = env.layout  # D: both sides (nearly: the agents' cancels) full at the end
        for off in (L.off_asks, L.off_bids):
            side = per_step[T - 1][e, off:off + 6 * L.n_orders].reshape(L.n_orders, 6)
            print("D", e, off, int((side[:, 0] != -1).sum()))
            assert (side[:, 0] != -1).sum() >= L.n_orders - 8


@pytest.mark.parametrize("T", [2, 3])
def test_quiet_volume_handover(T):
    """one and two lazy steps before the emitting step, metric config, 3 envs: the emitted arrays'
    volumes are those of the per-step launches (a carried best_q would be stale here)"""
    _rollout("2_player_fq_fqc", "gen", 3, T, True)


def test_quiet_volume_graph_replay():
    """the baked 5-env case captured in a HIP graph and replayed from the start state"""
    _rollout("2_player_fq_fqc", "gen", 5, 70, True, graph=True)
