"""hftlob_book_process_depth / hftlob_book_depth (k_book_process_depth, k_book_depth) and the
OrderBook wrapper on the GPU, bit-exact against the CPU oracle: the oracle's book_process called one
message at a time is the scan for cancel modes 0 and 1, and O.l2_state of each intermediate book is
the depth row after that message."""
import functools

import numpy as np
import pytest
import torch

from golden.book_scenarios import JORDERBOOK_EXPECT, JORDERBOOK_L2, JORDERBOOK_MSGS
from hftlob.config import JAXLOB_Configuration
from hftlob.engine import (book_process_, book_process_depth_, get_L2_state, scan_through_entire_array_save_states)
from hftlob.layout import pack_lob_cfg
from hftlob.orderbook import OrderBook
from oracle import pyoracle as O
from streams import (extreme_field_streams, full_book_messages, init_book_messages, noop_streams, random_streams,
                     top_streams)

pytestmark = pytest.mark.gpu

MAXINT = 2**31 - 1
GUARD, SENTINEL = 256, -777_777_777   # words before and after each per-message output array


def _empty(E, cfg):
    return np.full((E, cfg.nOrders, 6), -1, np.int32), np.full((E, cfg.nTrades, 8), -1, np.int32)


def _seeded(cfg, E, seed=3, init=None):
    e6, e8 = _empty(E, cfg)
    im = init_book_messages(E, seed=seed) if init is None else init
    a, b, _, _, _ = O.book_process(pack_lob_cfg(cfg), im, e6, e6, e8, save_best=False)
    return a, b, e8


def _replay(cfg, msgs, a0, b0, t0, n_levels):
    """The oracle, one message at a time: (all_asks, all_bids [E, M, nO, 6], depth [E, M, 4 L], a, b, t)."""
    lc = pack_lob_cfg(cfg)
    E, M = msgs.shape[:2]
    aa = np.zeros((E, M, cfg.nOrders, 6), np.int32)
    ab = np.zeros_like(aa)
    d = np.zeros((E, M, 4 * n_levels), np.int32)
    a, b, t = a0, b0, t0
    for k in range(M):
        a, b, t, _, _ = O.book_process(lc, np.ascontiguousarray(msgs[:, k:k + 1]), a, b, t, save_best=False)
        aa[:, k], ab[:, k] = a, b
        for e in range(E):
            d[e, k] = O.l2_state(lc, a[e], b[e], n_levels)
    return aa, ab, d, a, b, t


def _guarded(shape):
    n = int(np.prod(shape))
    flat = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device="cuda")
    return flat, flat[GUARD:GUARD + n].view(*shape)


def _gpu(cfg, msgs, a0, b0, t0, n_levels, n_keep=None, keys=None, sides=True, depth=True):
    """book_process_depth_ with every per-message output inside a guarded buffer:
    (depth [E, K, 4 L] | None, all_asks | None, all_bids | None, asks, bids, trades) as numpy."""
    E, M = msgs.shape[:2]
    K = M if n_keep is None else n_keep
    ga, gb, gt = (torch.from_numpy(x.copy()).cuda() for x in (a0, b0, t0))
    flats, gd, gaa, gab = [], None, None, None
    if depth:
        f, gd = _guarded((E, K, n_levels, 4))
        flats.append(f)
    if sides:
        f, gaa = _guarded((E, K, cfg.nOrders, 6))
        flats.append(f)
        f, gab = _guarded((E, K, cfg.nOrders, 6))
        flats.append(f)
    book_process_depth_(cfg, torch.from_numpy(msgs.copy()).cuda(), ga, gb, gt, n_levels, n_keep, gd, gaa, gab,
                        keys=None if keys is None else torch.from_numpy(keys.view(np.int32).copy()).cuda())
    torch.cuda.synchronize()
    for f in flats:
        f = f.cpu().numpy()
        assert (f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all(), "a write outside an output array"
        assert (f[GUARD:-GUARD] != SENTINEL).all(), "an output row was not written"
    out = [None if x is None else x.cpu().numpy() for x in (gd, gaa, gab, ga, gb, gt)]
    if out[0] is not None:
        out[0] = out[0].reshape(E, K, 4 * n_levels)
    return out


def _eq(name, want, got):
    bad = np.argwhere(want != got)
    assert bad.size == 0, f"{name} mismatch at {bad[:5].tolist()}: oracle {want[tuple(bad[0])]} gpu {got[tuple(bad[0])]}"


def _parity(cfg, msgs, a0, b0, t0, n_levels=10):
    want = _replay(cfg, msgs, a0, b0, t0, n_levels)
    d, aa, ab, a, b, t = _gpu(cfg, msgs, a0, b0, t0, n_levels)
    for name, w, g in zip(("all_asks", "all_bids", "depth", "asks", "bids", "trades"), want, (aa, ab, d, a, b, t)):
        _eq(name, w, g)
    pa, pb, pt = (torch.from_numpy(x.copy()).cuda() for x in (a0, b0, t0))
    book_process_(cfg, torch.from_numpy(msgs.copy()).cuda(), pa, pb, pt)
    for name, p, g in (("asks", pa, a), ("bids", pb, b), ("trades", pt, t)):
        assert np.array_equal(p.cpu().numpy(), g), f"final {name} differ from book_process_'s"
    return want, (d, aa, ab, a, b, t)


PARITY = {"default": {}, "t4_lim": dict(type_4_interpretation=1), "t4_mkt": dict(type_4_interpretation=2),
          "cancel0": dict(cancel_mode=0), "o16t8": dict(nOrders=16, nTrades=8), "o200t150": dict(nOrders=200, nTrades=150)}


@functools.lru_cache(maxsize=None)
def _parity_case(name):
    cfg = JAXLOB_Configuration(**PARITY[name])
    E, M = 16, 150
    a0, b0, t0 = _seeded(cfg, E)
    msgs = random_streams(E, M, seed=41)
    return cfg, _parity(cfg, msgs, a0, b0, t0)


# ----------------------------------------------------------------------------- hand golden
def test_jorderbook_hand_golden():
    """jorderbook.py:288-308: reset from the L2 snapshot, the two array messages, 10 levels"""
    ob = OrderBook()
    state = ob.reset(JORDERBOOK_L2)
    state, l2 = ob.process_orders_array_l2(state, JORDERBOOK_MSGS, 10)
    l2 = l2.cpu().numpy()
    assert l2.shape == (2, 40)
    asks = [(354200, 452), (361200, 100), (362900, 100), (364000, 400), (371900, 1100), (372200, 100), (372300, 200),
            (372800, 1000), (374600, 1000), (376700, 100)]
    bids = [(350100, 89), (346000, 99), (344000, 400), (343100, 100), (338700, 100), (337100, 1000), (336400, 1000),
            (336000, 300), (333600, 1000), (332500, 100)]
    row0 = np.array([[ap, aq, bp, bq] for (ap, aq), (bp, bq) in zip(asks, bids)], np.int32).ravel()
    row1 = row0.copy()
    row1[3] = 87
    assert np.array_equal(l2[0], row0) and np.array_equal(l2[1], row1)
    a, b, t = (x.cpu().numpy() for x in state[:3])
    for arr, rows in ((b, JORDERBOOK_EXPECT["bids_rows"]), (a, JORDERBOOK_EXPECT["asks_rows"]),
                      (t, JORDERBOOK_EXPECT["trades_rows"])):
        for i, r in rows.items():
            assert arr[i].tolist() == r, (i, arr[i].tolist(), r)
    # the carried key: PRNGKey(seed) split once by reset and once by the call (row 0 each time)
    k = np.array([[0, ob.cfg.seed]], np.uint32)
    for _ in range(2):
        k = O.split_keys(k, 2)[:, 0]
    assert np.array_equal(state.key.cpu().numpy().view(np.uint32), k[0])
    assert np.array_equal(ob.get_L2_state(state, 10).cpu().numpy(), row1)


# ----------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(PARITY))
def test_depth_parity_per_message(name):
    """E = 16, M = 150 (two full chunks and a 22-message tail), every message kept, 10 levels"""
    _parity_case(name)


@pytest.mark.parametrize("stream", ["top", "noop", "full", "extreme"])
def test_depth_parity_streams(stream):
    cfg = JAXLOB_Configuration()
    E, M = 16, 130
    init = full_book_messages(E, seed=8, lo=1.0) if stream == "full" else None
    a0, b0, t0 = _seeded(cfg, E, init=init)
    msgs = {"top": lambda: top_streams(E, M, seed=42), "noop": lambda: noop_streams(E, M, seed=43),
            "full": lambda: random_streams(E, M, seed=44), "extreme": lambda: extreme_field_streams(E, M, seed=45)}[stream]()
    if stream == "full":
        assert ((a0[..., 0] != -1).all(-1) | (b0[..., 0] != -1).all(-1)).any(), "no full side"
    want, _ = _parity(cfg, msgs, a0, b0, t0)
    if stream == "noop":
        d = want[2]
        assert (d[:, 1:] == d[:, :-1]).all(-1).mean() > 0.3, "few repeated rows"
    if stream == "extreme":
        assert (want[2] == -MAXINT).any() and (want[2] == MAXINT).any()


# ----------------------------------------------------------------------------- window edges
@pytest.mark.parametrize("n_keep", [1, 22, 23, 86, 87, 150])
def test_depth_window_edges(n_keep):
    """the window starts on the tail chunk's first message, one before it, and either side of the
    64 boundary: the last n_keep rows of the n_keep = M result"""
    cfg, (want, _) = _parity_case("default")
    E, M = 16, 150
    a0, b0, t0 = _seeded(cfg, E)
    msgs = random_streams(E, M, seed=41)
    d, aa, ab, a, b, t = _gpu(cfg, msgs, a0, b0, t0, 10, n_keep)
    _eq("depth", want[2][:, M - n_keep:], d)
    _eq("all_asks", want[0][:, M - n_keep:], aa)
    _eq("all_bids", want[1][:, M - n_keep:], ab)
    for name, w, g in zip(("asks", "bids", "trades"), want[3:], (a, b, t)):
        _eq(name, w, g)


@pytest.mark.parametrize("M", [1, 64, 65])
def test_depth_message_counts(M):
    cfg = JAXLOB_Configuration()
    a0, b0, t0 = _seeded(cfg, 16)
    _parity(cfg, np.ascontiguousarray(random_streams(16, 65, seed=46)[:, :M]), a0, b0, t0)


def test_depth_first_kept_is_noop():
    """a zero-quantity cancel in front: the first kept row is a skipped message's"""
    cfg = JAXLOB_Configuration()
    E = 16
    a0, b0, t0 = _seeded(cfg, E)
    msgs = random_streams(E, 70, seed=47)
    msgs[:, 0] = (2, 1, 0, 1000, 424242, 1, 34200, 0)
    want, _ = _parity(cfg, msgs, a0, b0, t0)
    lc = pack_lob_cfg(cfg)
    for e in range(E):
        assert np.array_equal(want[2][e, 0], O.l2_state(lc, a0[e], b0[e], 10))
    d = _gpu(cfg, msgs[:, :1].copy(), a0, b0, t0, 10)[0]
    _eq("depth", want[2][:, :1], d)


# ----------------------------------------------------------------------------- levels
@pytest.mark.parametrize("name", ["default", "o16t8"])
@pytest.mark.parametrize("n_levels", [1, 2, 15, 16])
def test_depth_levels(name, n_levels):
    cfg = JAXLOB_Configuration(**PARITY[name])
    E, M = 16, 70
    a0, b0, t0 = _seeded(cfg, E)
    msgs = random_streams(E, M, seed=48)
    want = _replay(cfg, msgs, a0, b0, t0, n_levels)
    d = _gpu(cfg, msgs, a0, b0, t0, n_levels, sides=False)[0]
    _eq("depth", want[2], d)


def test_depth_empty_book_fill_row():
    cfg = JAXLOB_Configuration()
    e6, e8 = _empty(4, cfg)
    msgs = np.zeros((4, 3, 8), np.int32)
    d = _gpu(cfg, msgs, e6, e6, e8, 16, sides=False)[0]
    assert (d.reshape(4, 3, 16, 4) == np.array([MAXINT, 0, -MAXINT, 0], np.int32)).all()
    l2 = get_L2_state(torch.from_numpy(e6).cuda(), torch.from_numpy(e6).cuda(), 16, cfg).cpu().numpy()
    assert (l2.reshape(4, 16, 4) == np.array([MAXINT, 0, -MAXINT, 0], np.int32)).all()


# ----------------------------------------------------------------------------- cancel modes 2 / 3
@pytest.mark.parametrize("mode,part", [(2, True), (3, True), (2, False)], ids=["random", "random_large", "legacy_threefry"])
def test_depth_random_cancel(mode, part):
    """message k draws from split(key, n_msg)[k], which one-message oracle calls do not reproduce:
    the final state against the oracle's whole scan, the last saved sides against the final sides,
    and every depth row against O.l2_state of its own saved sides"""
    cfg = JAXLOB_Configuration(cancel_mode=mode)
    E, M = 16, 150
    a0, b0, t0 = _seeded(cfg, E)
    msgs = top_streams(E, M, seed=49)   # (cancels at crowded best levels: the draw decides in every mode)
    keys = np.random.default_rng(mode).integers(0, 2**32, (E, 2), dtype=np.uint64).astype(np.uint32)
    lc = pack_lob_cfg(cfg, part)
    wa, wb, wt, _, _ = O.book_process(lc, msgs, a0, b0, t0, save_best=False, keys=keys)
    other = O.book_process(lc, msgs, a0, b0, t0, save_best=False, keys=np.zeros((E, 2), np.uint32))
    assert (other[0] != wa).any() or (other[1] != wb).any(), "the key never mattered"
    ga, gb, gt = (torch.from_numpy(x.copy()).cuda() for x in (a0, b0, t0))
    d = torch.empty((E, M, 10, 4), dtype=torch.int32, device="cuda")
    aa = torch.empty((E, M, cfg.nOrders, 6), dtype=torch.int32, device="cuda")
    ab = torch.empty_like(aa)
    book_process_depth_(cfg, torch.from_numpy(msgs).cuda(), ga, gb, gt, 10, None, d, aa, ab,
                        keys=torch.from_numpy(keys.view(np.int32).copy()).cuda(), prng_partitionable=part)
    torch.cuda.synchronize()
    for name, w, g in (("asks", wa, ga), ("bids", wb, gb), ("trades", wt, gt)):
        _eq(name, w, g.cpu().numpy())
    aa, ab, d = aa.cpu().numpy(), ab.cpu().numpy(), d.cpu().numpy().reshape(E, M, 40)
    _eq("all_asks[-1]", wa, aa[:, -1])
    _eq("all_bids[-1]", wb, ab[:, -1])
    for e in range(E):
        for k in range(M):
            assert np.array_equal(d[e, k], O.l2_state(lc, aa[e, k], ab[e, k], 10)), (e, k)


# ----------------------------------------------------------------------------- hftlob_book_depth
@pytest.mark.parametrize("name", list(PARITY))
def test_book_depth_operator(name):
    cfg, (want, got) = _parity_case(name)
    a, b = want[3], want[4]
    l2 = get_L2_state(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 10, cfg).cpu().numpy()
    _eq("get_L2_state", want[2][:, -1], l2)
    one = get_L2_state(torch.from_numpy(a[3]).cuda(), torch.from_numpy(b[3]).cuda(), 10, cfg).cpu().numpy()
    assert one.shape == (40,) and np.array_equal(one, l2[3])


def test_depth_empty_calls():
    """n_env = 0 and n_msg = 0 are no-ops; the n_msg = 0 call leaves the books untouched"""
    cfg = JAXLOB_Configuration()
    a0, b0, t0 = _seeded(cfg, 4)
    ga, gb, gt = (torch.from_numpy(x.copy()).cuda() for x in (a0, b0, t0))
    d = torch.full((4, 0, 10, 4), SENTINEL, dtype=torch.int32, device="cuda")
    book_process_depth_(cfg, torch.zeros((4, 0, 8), dtype=torch.int32, device="cuda"), ga, gb, gt, 10, None, d)
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")  # noqa: E731
    book_process_depth_(cfg, z(0, 5, 8), z(0, 100, 6), z(0, 100, 6), z(0, 100, 8), 10, None, z(0, 5, 10, 4))
    assert get_L2_state(z(0, 100, 6), z(0, 100, 6), 10, cfg).shape == (0, 40)
    # the ABI itself, with real buffers: nothing is written
    import ctypes as C
    from hftlob import _lib
    L, lc, s = _lib.lib(), pack_lob_cfg(cfg), _lib.stream_ptr()
    out = torch.full((4096,), SENTINEL, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    assert L.hftlob_book_process_depth(C.byref(lc), 4, 0, None, None, p(ga), p(gb), p(gt), 10, 0, p(out), None, None, s) == 0
    assert L.hftlob_book_process_depth(C.byref(lc), 0, 5, None, p(out), p(ga), p(gb), p(gt), 10, 5, p(out), None, None, s) == 0
    assert L.hftlob_book_depth(C.byref(lc), 0, 10, p(ga), p(gb), p(out), s) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    for w, g in ((a0, ga), (b0, gb), (t0, gt)):
        assert np.array_equal(w, g.cpu().numpy())


# ----------------------------------------------------------------------------- engine API
def test_engine_functional_forms():
    cfg, (want, _) = _parity_case("default")
    E, M = 16, 150
    a0, b0, t0 = _seeded(cfg, E)
    msgs = random_streams(E, M, seed=41)
    dev = [torch.from_numpy(x.copy()).cuda() for x in (msgs, a0, b0, t0)]
    before = [x.clone() for x in dev]
    aa, ab, t = scan_through_entire_array_save_states(cfg, None, dev[0], tuple(dev[1:]))
    a10, b10, t10 = scan_through_entire_array_save_states(cfg, None, dev[0], tuple(dev[1:]), N_steps=10)
    sa, sb, st = scan_through_entire_array_save_states(cfg, None, dev[0][5], tuple(x[5] for x in dev[1:]), N_steps=10)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(dev, before)), "an input was modified"
    _eq("all_asks", want[0], aa.cpu().numpy())
    _eq("all_bids", want[1], ab.cpu().numpy())
    _eq("trades", want[5], t.cpu().numpy())
    assert a10.shape == (E, 10, cfg.nOrders, 6) and torch.equal(a10, aa[:, -10:]) and torch.equal(b10, ab[:, -10:])
    assert torch.equal(t10, t)
    assert sa.shape == (10, cfg.nOrders, 6) and torch.equal(sa, a10[5]) and torch.equal(sb, b10[5]) and torch.equal(st, t[5])
    with pytest.raises(ValueError):
        scan_through_entire_array_save_states(cfg, None, dev[0], tuple(dev[1:]), N_steps=0)
    # the wrapper, batched: one launch gives the same rows and carries a key per env
    ob = OrderBook(cfg)
    s0 = ob.init(E)._replace(asks=dev[1], bids=dev[2])
    s1, l2 = ob.process_orders_array_l2(s0, dev[0], 10)
    _eq("l2_states", want[2], l2.cpu().numpy())
    assert torch.equal(s1.asks, aa[:, -1]) and torch.equal(s1.bids, ab[:, -1]) and s1.key.shape == (E, 2)
    assert all(torch.equal(x, y) for x, y in zip(dev, before)), "an input was modified"
    s2 = ob.process_orders_array(s0, dev[0])
    assert torch.equal(s2.asks, s1.asks) and torch.equal(s2.trades, s1.trades) and torch.equal(s2.key, s1.key)
