"""Inputs and guards of the engine's edge-size cases (test helper, CPU only): the sizes around the
kernels' 64-slot register sets (slot_sets: 1 / 2 / 4 sets for max(nOrders, nTrades) <= 64 / 128 /
256), books and trade logs filled up to their last rows, and the checks, computed from the
oracle's arrays alone, that a case really reached those rows.  The CPU tier pins oracle.c to
ref_py on these inputs, the GPU tier the HIP engine to oracle.c."""
import functools

import numpy as np

from hftlob.layout import pack_lob_cfg
from oracle import pyoracle as O
from streams import (EXTREME_VALUES, extreme_field_streams, filter_carry_streams, full_book_messages,  # noqa: F401
                     init_range_streams, prefilled_trades, random_streams, top_streams)

BOUNDARY_SIZES = [(63, 63), (64, 64), (65, 65), (127, 127), (128, 128), (129, 129)]
TRADES_LARGER = [(64, 65), (16, 129), (2, 129), (100, 200)]      # the slot sets come from nTrades
ORDERS_LARGER = [(65, 64), (129, 1), (200, 8)]                   # ... from nOrders
TINY_SIZES = [(1, 1), (2, 1), (1, 2), (3, 2)]
EDGE_SIZES = BOUNDARY_SIZES + TRADES_LARGER + ORDERS_LARGER + TINY_SIZES

INT32_MIN = -2**31
# book_depth / init_id away from 10 / -2 (get_init_id_match's id range [init_id - 2 * book_depth, init_id])
INIT_RANGE_CASES = [dict(book_depth=0), dict(book_depth=3), dict(init_id=-12), dict(init_id=INT32_MIN + 20)]


def slot_sets(nO, nT):
    n = max(nO, nT)
    return 1 if n <= 64 else 2 if n <= 128 else 4


@functools.lru_cache(maxsize=None)
def _edge_messages(E, M):
    return np.concatenate([random_streams(E, M // 2, seed=101), top_streams(E, M - M // 2, seed=102)], axis=1)


def edge_messages(E, M):
    """random_streams then top_streams (M // 2 messages each): generated once, every size gets a copy"""
    return _edge_messages(E, M).copy()


def empty_book(E, cfg):
    return np.full((E, cfg.nOrders, 6), -1, np.int32), np.full((E, cfg.nTrades, 8), -1, np.int32)


def full_books(cfg, E, seed, **kw):
    """both sides 85-100 % full (full_book_messages through the oracle)"""
    e6, e8 = empty_book(E, cfg)
    init = full_book_messages(E, seed=seed, nO=cfg.nOrders, **kw)
    a0, b0, _, _, _ = O.book_process(pack_lob_cfg(cfg), init, e6, e6, e8, save_best=False)
    return a0, b0


def occupied(x, row):
    """envs whose row `row` of a side / trade log holds anything but -1"""
    return (x[:, row] != -1).any(axis=-1)


def assert_side_edges(nO, starts, ends):
    """some env holds an order in row nO - 1, and in the rows on both sides of every 64-slot
    boundary below nO, on each side of the book, at the start or the end of a run"""
    rows = {nO - 1} | {r for r in (63, 64, 127, 128) if r < nO}
    for name, idx in (("asks", 0), ("bids", 1)):
        for r in sorted(rows):
            hit = any(occupied(run[idx], r).any() for run in list(starts) + list(ends))
            assert hit, f"no env holds an order in {name} row {r} (nOrders {nO}): the edge was not exercised"


def assert_trade_edge(nT, trades_end):
    assert occupied(trades_end, nT - 1).any(), f"no env wrote trade row {nT - 1}: the edge was not exercised"


def init_range_inputs(cfg, E, seed):
    """(books, streams) of a book_depth / init_id case: 85-100 % full books a third of whose orders
    carry cfg.init_id, then init_range_streams (adds and cancels around the id range's two ends)
    and filter_carry_streams"""
    a0, b0 = full_books(cfg, E, seed, init_id=cfg.init_id)
    return (a0, b0), {"init_range": init_range_streams(E, 256, seed + 1, init_id=cfg.init_id, nO=cfg.nOrders),
                      "filter_carry": filter_carry_streams(E, seed + 2)}
