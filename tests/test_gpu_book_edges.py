"""Engine parity at the edges the size-templated kernels change shape at: HIP hftlob_book_process
vs the CPU oracle, bit-exact, at the 64-slot register-set boundaries (k_book_process<S, RC>: S = 1 /
2 / 4 for max(nOrders, nTrades) <= 64 / 128 / 256), unequal and tiny sizes, the chunk loop's message
counts, the form without best-quote arrays, book_depth / init_id away from their defaults and
message fields at int32's extremes.  Every size case asserts, from the oracle's arrays alone, that
the last rows were really reached (book_edges)."""
import functools

import numpy as np
import pytest
import torch

import book_edges as X
from hftlob.config import JAXLOB_Configuration
from hftlob.engine import book_process_, scan_through_entire_array, scan_through_entire_array_save_bidask
from hftlob.layout import pack_lob_cfg
from oracle import pyoracle as O
from streams import init_book_messages, random_streams, top_streams
from test_gpu_book import _run

pytestmark = pytest.mark.gpu

N_ENV, N_MSG = 64, 400


def _size_case(nO, nT, **kw):
    """from 85-100 % full books with an empty trade log, then from empty books with a trade log
    filled up to its last two rows; the guards over both runs"""
    cfg = JAXLOB_Configuration(nOrders=nO, nTrades=nT, **kw)
    msgs = X.edge_messages(N_ENV, N_MSG)
    e6, e8 = X.empty_book(N_ENV, cfg)
    a0, b0 = X.full_books(cfg, N_ENV, seed=9)
    r1 = _run(cfg, msgs, a0, b0, e8)
    r2 = _run(cfg, msgs, e6, e6, X.prefilled_trades(N_ENV, nT, seed=5))
    X.assert_side_edges(nO, [(a0, b0)], [r1[:2], r2[:2]])
    X.assert_trade_edge(nT, r2[2])


@pytest.mark.parametrize("nO,nT", X.EDGE_SIZES, ids=lambda v: str(v))
def test_book_edge_sizes(nO, nT):
    """63/64/65 and 127/128/129 slots and trade rows (the Valid<S> masks, first_slot's fallback
    nO - 1, the -1 -> last slot wrap and the column over-reads at a register-set boundary), sizes
    whose slot sets come from the trade log (nTrades > nOrders) or from the book alone (129/1:
    the widest over-read past the shortest log), and books of 1 to 3 slots."""
    _size_case(nO, nT)


@pytest.mark.parametrize("kw", [dict(type_4_interpretation=1), dict(cancel_mode=2)], ids=str)
@pytest.mark.parametrize("nO,nT", X.BOUNDARY_SIZES, ids=lambda v: str(v))
def test_book_boundary_sizes_modes(nO, nT, kw):
    """LIM type-4 messages (the remainder rests: fuller books) and the random cancel fallback
    (k_book_process<S, true>: the draw over a side's price-matched rows) at the boundary sizes"""
    _size_case(nO, nT, **kw)


# ------------------------------------------------------------ message counts
MSG_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193]
GUARD, SENTINEL = 128, -777_777_777   # words before and after each best-quote array


@functools.lru_cache(maxsize=None)
def _long_stream(E):
    out = np.concatenate([random_streams(E, 100, seed=61), top_streams(E, 93, seed=62)], axis=1)
    out.setflags(write=False)
    return out


def _guarded_run(cfg, msgs, a0, b0, t0, keys=None):
    """_run's comparison with the best-quote arrays inside flat buffers that carry GUARD sentinel
    words before the first env's rows and after the last env's: rows [e * n_msg, (e + 1) * n_msg)
    are env e's (the ABI's arrays are contiguous, so a write past an env's last row lands in the
    next env's rows, which the parity check sees, or in the guard)."""
    E, M = msgs.shape[:2]
    lc = pack_lob_cfg(cfg)
    oa, ob, ot, oba, obb = O.book_process(lc, msgs, a0, b0, t0, keys=keys)
    ga, gb, gt = (torch.from_numpy(x.copy()).cuda() for x in (a0, b0, t0))
    flat = [torch.full((2 * GUARD + E * M * 2,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)]
    gba, gbb = (f[GUARD:GUARD + E * M * 2].view(E, M, 2) for f in flat)
    book_process_(cfg, torch.from_numpy(msgs.copy()).cuda(), ga, gb, gt, gba, gbb,
                  keys=None if keys is None else torch.from_numpy(keys.view(np.int32)).cuda())
    torch.cuda.synchronize()
    for name, o, g in (("asks", oa, ga), ("bids", ob, gb), ("trades", ot, gt), ("best_asks", oba, gba),
                       ("best_bids", obb, gbb)):
        g = g.cpu().numpy()
        bad = np.argwhere(o != g)
        assert bad.size == 0, f"{name} mismatch at {bad[:5].tolist()}: oracle {o[tuple(bad[0])]} gpu {g[tuple(bad[0])]}"
    for f in flat:
        f = f.cpu().numpy()
        assert (f[:GUARD] == SENTINEL).all() and (f[GUARD + E * M * 2:] == SENTINEL).all(), \
            "a write outside the best-quote array"


def _count_case(nO, nT, n_msg, E=48, **kw):
    cfg = JAXLOB_Configuration(nOrders=nO, nTrades=nT, **kw)
    e6, e8 = X.empty_book(E, cfg)
    a0, b0, _, _, _ = O.book_process(pack_lob_cfg(cfg), init_book_messages(E, seed=3), e6, e6, e8, save_best=False)
    msgs = np.ascontiguousarray(_long_stream(E)[:, :n_msg])
    keys = None
    if cfg.cancel_mode >= 2:
        keys = np.random.default_rng(n_msg).integers(0, 2**32, (E, 2), dtype=np.uint64).astype(np.uint32)
    _guarded_run(cfg, msgs, a0, b0, e8, keys)


@pytest.mark.parametrize("n_msg", MSG_COUNTS)
@pytest.mark.parametrize("nO,nT", [(100, 100), (40, 30)], ids=lambda v: str(v))
def test_book_message_counts(nO, nT, n_msg):
    """Prefixes of one stream around the 64-message chunk: the one-chunk-ahead prefetch
    (row + 64 < n_msg), the last chunk's count min(64, n_msg - base) and the row < n_msg store of
    the best quotes, which must not write outside its [E, n_msg, 2] arrays."""
    _count_case(nO, nT, n_msg)


@pytest.mark.parametrize("n_msg", [1, 64, 65])
@pytest.mark.parametrize("nO,nT", [(100, 100), (40, 30)], ids=lambda v: str(v))
def test_book_message_counts_random_cancel(nO, nT, n_msg):
    """cancel_mode 3: message k draws from split(key, n_msg)[k], so each prefix is another draw"""
    _count_case(nO, nT, n_msg, cancel_mode=3)


# ------------------------------------------------------------ no best-quote arrays
@pytest.mark.parametrize("single", [False, True], ids=["batched", "single"])
@pytest.mark.parametrize("mode", [1, 2])
def test_book_null_best_form(mode, single):
    """scan_through_entire_array (best_asks == best_bids == NULL in the ABI): books and trades equal
    the oracle's and scan_through_entire_array_save_bidask's on the same input, which is left
    unmodified; batched and single-env input, cancel_mode 1 and 2 (one key for every env)."""
    cfg = JAXLOB_Configuration(cancel_mode=mode)
    E, M = (1, 150) if single else (24, 150)
    e6, e8 = X.empty_book(E, cfg)
    a0, b0, t0, _, _ = O.book_process(pack_lob_cfg(cfg), init_book_messages(E, seed=12), e6, e6, e8, save_best=False)
    msgs = top_streams(E, M, seed=71)
    key = np.array([0x9E3779B9, 0x12345678], np.uint32)
    want = O.book_process(pack_lob_cfg(cfg), msgs, a0, b0, t0, keys=np.broadcast_to(key, (E, 2)))
    if mode == 2:
        other = O.book_process(pack_lob_cfg(cfg), msgs, a0, b0, t0, keys=np.zeros((E, 2), np.uint32))
        assert single or any((x != y).any() for x, y in zip(want[:3], other[:3])), "the key never mattered"
    pick = (lambda x: x[0]) if single else (lambda x: x)  # noqa: E731
    dev = [torch.from_numpy(pick(x).copy()).cuda() for x in (msgs, a0, b0, t0)]
    before = [x.clone() for x in dev]
    k = torch.from_numpy(key.astype(np.int64)).cuda()
    got = scan_through_entire_array(cfg, k, dev[0], tuple(dev[1:]))
    got2, (ba, bb) = scan_through_entire_array_save_bidask(cfg, k, dev[0], tuple(dev[1:]))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(dev, before)), "an input was modified"
    for name, o, g, g2 in zip(("asks", "bids", "trades"), want[:3], got, got2):
        assert g.shape == pick(o).shape
        assert np.array_equal(g.cpu().numpy(), pick(o)), f"{name} differ from the oracle's"
        assert torch.equal(g, g2), f"{name} differ from the save_bidask form's"
    assert np.array_equal(ba.cpu().numpy(), pick(want[3])) and np.array_equal(bb.cpu().numpy(), pick(want[4]))


# ------------------------------------------------------------ book_depth / init_id
@pytest.mark.parametrize("kw", X.INIT_RANGE_CASES, ids=str)
@pytest.mark.parametrize("nO,nT", [(100, 100), (40, 30)], ids=lambda v: str(v))
def test_book_init_id_range(nO, nT, kw):
    """book_depth 0 / 3 and init_id -12 / INT32_MIN + 20 (get_init_id_match's id range
    [init_id - 2 * book_depth, init_id], which the no-op pre-pass reasons about too): over 85-100 %
    full books a third of whose orders carry the init id, streams.init_range_streams (adds and
    cancels at both ends of the range) and filter_carry_streams.  The setting must matter: the
    oracle's books under the default book_depth 10 / init_id -2 differ on the same input."""
    cfg = JAXLOB_Configuration(nOrders=nO, nTrades=nT, **kw)
    dflt = pack_lob_cfg(JAXLOB_Configuration(nOrders=nO, nTrades=nT))
    E = 64
    (a0, b0), streams = X.init_range_inputs(cfg, E, seed=17 + nO)
    _, e8 = X.empty_book(E, cfg)
    for name, msgs in streams.items():
        oa, ob = _run(cfg, msgs, a0, b0, e8)[:2]
        da, db, _, _, _ = O.book_process(dflt, msgs, a0, b0, e8)
        assert (da != oa).any() or (db != ob).any(), f"{kw} never changed the result on {name}"


# ------------------------------------------------------------ extreme fields
@pytest.mark.parametrize("t4", [0, 1, 2], ids=["ioc", "lim", "mkt"])
@pytest.mark.parametrize("nO,nT", [(100, 100), (16, 8), (65, 65)], ids=lambda v: str(v))
def test_book_extreme_fields(nO, nT, t4):
    """Order ids, prices, seconds and nanoseconds at INT32_MIN, INT32_MIN + 1, INT32_MAX - 1,
    INT32_MAX, 0, -1, -2, -22 and -23 (streams.extreme_field_streams; quantities up to 2^22, inside
    int32 arithmetic): the decode's sign tests, the filter's hashes of ids and prices, the
    top-of-book time comparisons and the type-4 price substitutions, from seeded and empty books."""
    cfg = JAXLOB_Configuration(nOrders=nO, nTrades=nT, type_4_interpretation=t4)
    E, M = 64, 400
    msgs = X.extreme_field_streams(E, M, seed=19 + nO)
    for col in (3, 4, 6, 7):
        assert set(X.EXTREME_VALUES) <= set(msgs[..., col].ravel().tolist())
    e6, e8 = X.empty_book(E, cfg)
    a0, b0, _, _, _ = O.book_process(pack_lob_cfg(cfg), init_book_messages(E, seed=6), e6, e6, e8, save_best=False)
    _run(cfg, msgs, a0, b0, e8)
    _run(cfg, msgs, e6, e6, e8)
