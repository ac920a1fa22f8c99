"""The depth entry points' ABI surface and the OrderBook wrapper's host side, without a GPU: the
declarations and exports, the argument checks (which run before any device work), init_msgs_from_l2,
the quote-dict mapping, and every torch query on CPU tensors against a numpy restatement written
from the cited lines of gymnax_exchange/jaxob/JaxOrderBookArrays.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from golden.book_scenarios import JORDERBOOK_L2, jorderbook_init_msgs
from hftlob import _lib
from hftlob.config import JAXLOB_Configuration
from hftlob.layout import pack_lob_cfg
from hftlob.orderbook import LobState, OrderBook, init_msgs_from_l2, quote_to_msg
from oracle import pyoracle as O
from streams import init_book_messages, random_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hftlob_book_depth", "hftlob_book_process_depth")
MAXINT = 2**31 - 1


# ------------------------------------------------------------------------------- ABI
def test_new_entry_points_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "hftlob.h")).read()
    declared = set(re.findall(r"\b(hftlob_[a-z_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS
    assert re.search(r"#define\s+HFTLOB_MAX_DEPTH_LEVELS\s+16\b", src)
    assert re.search(r"#define\s+HFTLOB_ABI_VERSION\s+8\b", src)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= syms


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built")
    return _lib.lib()


def test_depth_argument_checks(L):
    """hftlob.h's error surface: every check before any device work (the pointers are dummies)"""
    lob = pack_lob_cfg(JAXLOB_Configuration())
    c, k = C.byref(lob), C.c_void_p(64)
    P = L.hftlob_book_process_depth
    # (cfg, n_env, n_msg, keys, msgs, asks, bids, trades, n_levels, n_keep, depth, all_asks, all_bids, stream)
    assert P(None, 4, 8, None, k, k, k, k, 10, 8, k, None, None, None) == -2           # null cfg
    assert P(c, -1, 8, None, k, k, k, k, 10, 8, k, None, None, None) == -3             # negative n_env
    for n_levels in (0, 17, -1):
        assert P(c, 4, 8, None, k, k, k, k, n_levels, 8, k, None, None, None) == -3    # n_levels outside 1..16
    assert b"n_levels" in L.hftlob_last_error()
    for n_keep in (0, 9, -1):
        assert P(c, 4, 8, None, k, k, k, k, 10, n_keep, k, None, None, None) == -3     # n_keep outside 1..n_msg
    assert b"n_keep" in L.hftlob_last_error()
    assert P(c, 4, 8, None, k, k, k, k, 10, 8, None, None, None, None) == -2           # no output at all
    assert P(c, 4, 8, None, k, k, k, k, 10, 8, k, k, None, None) == -2                 # all_asks alone
    assert P(c, 4, 8, None, k, k, k, k, 10, 8, None, None, k, None) == -2              # all_bids alone
    assert b"both or none" in L.hftlob_last_error()
    assert P(c, 4, 8, None, None, k, k, k, 10, 8, k, None, None, None) == -2           # null msgs
    assert P(c, 4, 8, None, k, None, k, k, 10, 8, k, None, None, None) == -2           # null asks
    assert P(c, 0, 8, None, None, None, None, None, 10, 8, k, None, None, None) == 0   # empty batch
    assert P(c, 4, 0, None, None, None, None, None, 10, 0, k, None, None, None) == 0   # no messages
    lob.cancel_mode = 2
    assert P(c, 4, 8, None, k, k, k, k, 10, 8, k, None, None, None) == -2              # keys required
    assert b"keys" in L.hftlob_last_error()
    lob.cancel_mode = 1
    D = L.hftlob_book_depth
    assert D(None, 4, 10, k, k, k, None) == -2
    assert D(c, -1, 10, k, k, k, None) == -3
    for n_levels in (0, 17):
        assert D(c, 4, n_levels, k, k, k, None) == -3
    assert D(c, 4, 10, None, k, k, None) == -2 and D(c, 4, 10, k, k, None, None) == -2
    assert D(c, 0, 10, None, None, None, None) == 0
    lob.n_orders = 0
    assert D(c, 4, 10, k, k, k, None) == -3 and P(c, 4, 8, None, k, k, k, k, 10, 8, k, None, None, None) == -3


def test_engine_rejects_before_the_library():
    from hftlob.engine import book_process_depth_, get_L2_state, scan_through_entire_array_save_states
    cfg = JAXLOB_Configuration()
    z = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    msgs, a, t = z(2, 5, 8), z(2, 100, 6), z(2, 100, 8)
    with pytest.raises(ValueError, match="n_keep"):
        book_process_depth_(cfg, msgs, a, a, t, 10, 6, z(2, 6, 10, 4))
    with pytest.raises(ValueError, match="n_levels"):
        book_process_depth_(cfg, msgs, a, a, t, 17, 5, z(2, 5, 17, 4))
    with pytest.raises(ValueError, match="depth must be"):
        book_process_depth_(cfg, msgs, a, a, t, 10, 5, z(2, 5, 40))
    with pytest.raises(ValueError, match="both or none"):
        book_process_depth_(cfg, msgs, a, a, t, 10, 5, None, z(2, 5, 100, 6), None)
    with pytest.raises(ValueError, match="give depth"):
        book_process_depth_(cfg, msgs, a, a, t, 10, 5)
    with pytest.raises(ValueError, match="N_steps"):
        scan_through_entire_array_save_states(cfg, None, msgs, (a, a, t), N_steps=0)
    with pytest.raises(ValueError, match="n_levels"):
        get_L2_state(a, a, 0, cfg)


# ------------------------------------------------------------------------------- messages
def test_init_msgs_from_l2():
    cfg = JAXLOB_Configuration()
    got = init_msgs_from_l2(cfg, JORDERBOOK_L2, time=[0, 0])
    assert got.dtype == torch.int32 and got.tolist() == jorderbook_init_msgs()
    dflt = init_msgs_from_l2(cfg, JORDERBOOK_L2)
    assert (dflt[:, 6] == 34200).all() and (dflt[:, 7] == 0).all() and torch.equal(dflt[:, :6], got[:, :6])
    two = init_msgs_from_l2(cfg, [JORDERBOOK_L2, JORDERBOOK_L2[::-1]], time=[[0, 0], [7, 9]])
    assert torch.equal(two[0], got) and two[1, :, 6:].tolist() == [[7, 9]] * 20
    assert two[1, :, 3].tolist() == JORDERBOOK_L2[::-1][0::2] and two[1, :, 2].tolist() == JORDERBOOK_L2[::-1][1::2]


@pytest.mark.parametrize("typ,side,want", [
    ("limit", "bid", (1, 1)), ("limit", "ask", (1, -1)), ("cancel", "bid", (2, 1)), ("cancel", "ask", (2, -1)),
    ("delete", "bid", (2, 1)), ("delete", "ask", (2, -1)), ("market", "bid", (1, -1)), ("market", "ask", (1, 1)),
    ("modify", "bid", (5, 1)), ("modify", "sell", (5, -1))])
def test_quote_dict_mapping(typ, side, want):
    """jorderbook.py:64-91: trade_id before order_id, the 's.ns' timestamp string"""
    q = {'type': typ, 'side': side, 'quantity': 99, 'price': 346000, 'trade_id': 8888, 'order_id': 7777,
         'timestamp': '3400.005000000'}
    assert quote_to_msg(q) == [want[0], want[1], 99, 346000, 8888, 7777, 3400, 5000000]


# ------------------------------------------------------------------------------- queries
def _np_unique_fill(x, size, fill):
    u = np.unique(x)[:size]
    return np.concatenate([u, np.full(size - u.size, fill, x.dtype)])


def _np_first(side, m):
    i = np.flatnonzero(m)
    return side[i[0]] if i.size else np.full(6, -99, np.int32)


def _np_top(cfg, side, s):
    """_get_top_{ask,bid}_order_idx — :241-268"""
    p = s[:, 0]
    best = np.where(p == -1, cfg.maxint, p).min() if side == 0 else p.max()
    times = np.where(p == best, s[:, 4], cfg.maxint)
    tns = np.where(times == times.min(), s[:, 5], cfg.maxint)
    return s[np.flatnonzero(tns == tns.min())[0]]


def _books(nO):
    """oracle-produced books [E = 8 + 3]: seeded + random streams, then an empty book, a side full
    of one price and a side whose rows share one time"""
    cfg = JAXLOB_Configuration(nOrders=nO, nTrades=nO)
    E = 8
    e6 = np.full((E, nO, 6), -1, np.int32)
    e8 = np.full((E, nO, 8), -1, np.int32)
    lc = pack_lob_cfg(cfg)
    a, b, t, _, _ = O.book_process(lc, init_book_messages(E, seed=5), e6, e6, e8, save_best=False)
    a, b, t, _, _ = O.book_process(lc, random_streams(E, 200, seed=6), a, b, t, save_best=False)
    one = np.array([[1000, 3 + i, 50 + i % 3, 4, 34200 + (i % 2), 7 - i % 5] for i in range(nO)], np.int32)
    tie = one.copy()
    tie[:, 0] = 1000 + np.arange(nO) % 3
    tie[:, 4:] = (34200, 5)
    a = np.concatenate([a, e6[:1], one[None], tie[None]])
    b = np.concatenate([b, e6[:1], one[None], tie[None]])
    return cfg, a, b


@pytest.mark.parametrize("nO", [100, 16])
def test_queries_against_numpy(nO):
    cfg, a, b = _books(nO)
    E = a.shape[0]
    ob = OrderBook(cfg, device="cpu")
    st = LobState(torch.from_numpy(a), torch.from_numpy(b), torch.full((E, nO, 8), -1, dtype=torch.int32),
                  torch.zeros((E, 2), dtype=torch.int32))
    hit = {"found": 0, "missing": 0, "fallback": 0, "both": 0}
    for side, arr in ((0, a), (1, b)):
        ids = ob.get_side_ids(st, side).numpy()
        vol = ob.get_volume(st, side).numpy()
        nxt = ob.get_next_executable_order(st, side).numpy()
        best = ob.get_best_price(st, side).numpy()
        for e in range(E):
            s = arr[e]
            p, q = s[:, 0], s[:, 1]
            assert np.array_equal(ids[e], _np_unique_fill(s[:, 2], nO, 1))                       # :1200-1209
            assert vol[e] == np.where(p != -1, q, 0).sum()                                         # :919-930
            assert np.array_equal(nxt[e], _np_top(cfg, side, s))                                   # :1211-1229
            if side == 0:                                                                          # :932-951
                mn = np.where(p == -1, cfg.maxint, p).min()
                assert best[e] == (-1 if mn == cfg.maxint else mn)
            else:
                assert best[e] == p.max()
            one = LobState(st.asks[e], st.bids[e], st.trades[e], st.key[e])                        # single form
            assert np.array_equal(ob.get_next_executable_order(one, side).numpy(), nxt[e])
            assert int(ob.get_best_price(one, side)) == best[e]
            for price in sorted(set(p[:5].tolist()) | {-1, 999_999}):
                got = int(ob.get_volume_at_price(one, side, price))
                assert got == np.where(p == price, q, 0).sum()                                     # :906-917
                m = (p == price) & (s[:, 2] <= cfg.init_id) & (s[:, 2] >= cfg.init_id - 2 * cfg.book_depth)
                assert int(ob.get_volume_at_price(one, side, price, init_only=True)) == np.where(m, q, 0).sum()  # :1030-1046
            rows = [s[0], s[nO // 2], s[-1], np.array([123456, 1, 987654, 555, 1, 2], np.int32)]
            for r in rows:
                pr, oid, tid, ts, tns = (int(r[i]) for i in (0, 2, 3, 4, 5))
                w = _np_first(s, s[:, 2] == oid)                                                   # :1048-1071
                hit["found" if (s[:, 2] == oid).any() else "missing"] += 1
                assert np.array_equal(ob.get_order(one, side, oid).numpy(), w)
                assert np.array_equal(ob.get_order(one, side, oid, pr + 1).numpy(),
                                      _np_first(s, (s[:, 2] == oid) & (p == pr + 1)))              # :1099-1124
                assert np.array_equal(ob.get_order(one, side, oid, pr).numpy(), _np_first(s, (s[:, 2] == oid) & (p == pr)))
                assert np.array_equal(ob.get_order_by_tid(one, side, tid).numpy(), _np_first(s, s[:, 3] == tid))  # :1074-1097
                at = (s[:, 4] == ts) & (s[:, 5] == tns)
                assert np.array_equal(ob.get_order_at_time(one, side, ts, tns).numpy(), _np_first(s, at))  # :1127-1154
                for price in (pr, pr + 1):                                                         # :1156-1198
                    m = at & (p == price)
                    hit["both" if m.any() else "fallback"] += 1
                    assert np.array_equal(ob.get_order_at_time(one, side, ts, tns, price).numpy(),
                                          _np_first(s, m if m.any() else at))
        # the batched form of a lookup agrees with the per-env one
        oid = torch.from_numpy(arr[:, 1, 2].copy())
        got = ob.get_order(st, side, oid.unsqueeze(-1)).numpy()
        for e in range(E):
            assert np.array_equal(got[e], _np_first(arr[e], arr[e][:, 2] == arr[e, 1, 2]))
    assert all(v > 0 for v in hit.values()), hit
    ba, bb = ob.get_best_bid_and_ask_inclQuants(st)                                                # :967-984
    for e in range(E):
        pa, pb = a[e][:, 0], b[e][:, 0]
        mn = np.where(pa == -1, cfg.maxint, pa).min()
        wa = -1 if mn == cfg.maxint else mn
        assert ba[e].tolist() == [wa, np.where(pa == wa, a[e][:, 1], 0).sum()]
        assert bb[e].tolist() == [pb.max(), np.where(pb == pb.max(), b[e][:, 1], 0).sum()]
    for bad in (2, -1):
        with pytest.raises(ValueError):
            ob.get_volume(st, bad)
        with pytest.raises(ValueError):
            ob.get_next_executable_order(st, bad)
        with pytest.raises(ValueError):
            ob.get_best_price(st, bad)


def test_init_state_and_key():
    ob = OrderBook(JAXLOB_Configuration(nOrders=16, nTrades=8), device="cpu")
    s = ob.init()
    assert s.asks.shape == (16, 6) and s.trades.shape == (8, 8) and (s.asks == -1).all() and (s.trades == -1).all()
    assert s.key.tolist() == [0, ob.cfg.seed]
    s = ob.init(3)
    assert s.bids.shape == (3, 16, 6) and s.key.tolist() == [[0, ob.cfg.seed]] * 3
    with pytest.raises(RuntimeError, match="device"):
        ob.reset(JORDERBOOK_L2[:8])   # processing needs the GPU library: no host fall-back
