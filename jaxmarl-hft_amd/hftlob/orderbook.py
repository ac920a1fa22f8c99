"""The order-book object: ``gymnax_exchange/jaxob/jorderbook.py:17-268`` on device tensors.

``LobState(asks, bids, trades, key)`` and ``OrderBook(cfg)`` with the reference's methods.  The
processing methods launch the engine kernels (``hftlob.engine``); ``process_orders_array_l2`` is one
``hftlob_book_process_depth`` launch that replays the messages and returns the L2 depth after each.
The queries are torch ops on whatever device the state lives on: no host synchronisation and no
Python branch on a tensor's value, so they can sit inside a captured graph.

Every array may carry a leading env dimension (the reference is one book; ``jax.vmap`` is the
explicit batch here): asks / bids ``[E, nO, 6]``, trades ``[E, nT, 8]``, key ``[2]`` or ``[E, 2]``
(int32 words holding the uint32 key).  ``side`` is 0 = asks, 1 = bids as in the wrapper; anything
else raises ``ValueError``.

Keys: each processing call does ``key, sub = jax.random.split(key)`` (jorderbook.py:93,107,119,130);
``key`` is carried on and ``sub`` is the scan's key.  Only cancel modes 2 / 3 draw from it, where
message k of a scan of M draws from ``split(sub, M)[k]``.  One deviation: the reference's
single-message methods hand ``sub`` itself to the message; here a single message is a scan of one,
so it draws from ``split(sub, 1)[0]``.

Not carried over: ``LOBSTER_INTERPRETER`` mode (it raises in the reference) and the
``jax.tree_util`` registration.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import constants as cst
from . import engine
from .config import JAXLOB_Configuration


class LobState(NamedTuple):
    asks: torch.Tensor
    bids: torch.Tensor
    trades: torch.Tensor
    key: torch.Tensor


def init_msgs_from_l2(cfg: JAXLOB_Configuration, book_l2, time=None, device=None) -> torch.Tensor:
    """init_msgs_from_l2 — JaxOrderBookArrays.py:999-1028: the limit orders that rebuild an L2
    snapshot [ask_p, ask_q, bid_p, bid_q, ...] (or [E, 4 * levels]): even rows asks, odd rows bids,
    order id init_id - k, trader id init_id, time [s, ns] (default [34200, 0])."""
    l2 = torch.as_tensor(book_l2, device=device).to(torch.int32)
    levels = l2.shape[-1] // 4
    data = l2.reshape(l2.shape[:-1] + (levels * 2, 2))
    t = torch.as_tensor([34200, 0] if time is None else time, device=l2.device).to(torch.int32)
    k = torch.arange(levels * 2, dtype=torch.int32, device=l2.device)
    msgs = torch.zeros(l2.shape[:-1] + (levels * 2, 8), dtype=torch.int32, device=l2.device)
    msgs[..., 0] = 1
    msgs[..., 1] = torch.where(k % 2 == 0, -1, 1).to(torch.int32)
    msgs[..., 2] = data[..., 1]
    msgs[..., 3] = data[..., 0]
    msgs[..., 4] = cfg.init_id - k
    msgs[..., 5] = cfg.init_id
    msgs[..., 6] = t[..., 0:1]
    msgs[..., 7] = t[..., 1:2]
    return msgs


def quote_to_msg(quote: Dict) -> list:
    """The message row of a quote dict — jorderbook.py:64-91:
    [type, side, quantity, price, trade_id, order_id, s, ns] (trade_id before order_id, sic)."""
    inttype = 5
    intside = -1
    if quote['side'] == 'bid':
        intside = 1
    if quote['type'] == 'limit':
        inttype = 1
    elif quote['type'] == 'cancel':
        inttype = 2
    elif quote['type'] == 'delete':
        inttype = 2
    elif quote['type'] == 'market':
        inttype = 1
        intside = intside * -1
    s, ns = quote['timestamp'].split('.')[:2]
    return [inttype, intside, int(quote['quantity']), int(quote['price']), int(quote['trade_id']),
            int(quote['order_id']), int(s), int(ns)]


# ------------------------------------------------------------------ queries (torch, any device)
def _side(state: LobState, side: int) -> torch.Tensor:
    if side == 0:
        return state.asks
    if side == 1:
        return state.bids
    raise ValueError('Side must be 0 or 1')


def get_volume_at_price(orderside: torch.Tensor, price) -> torch.Tensor:
    """JaxOrderBookArrays.py:906-917 (int32 sum, wrapping)."""
    q = torch.where(orderside[..., 0] == price, orderside[..., 1], 0)
    return q.sum(-1, dtype=torch.int32)


def get_init_volume_at_price(orderside: torch.Tensor, price, cfg: JAXLOB_Configuration) -> torch.Tensor:
    """JaxOrderBookArrays.py:1030-1046."""
    oid = orderside[..., 2]
    m = (orderside[..., 0] == price) & (oid <= cfg.init_id) & (oid >= cfg.init_id - cfg.book_depth * 2)
    return torch.where(m, orderside[..., 1], 0).sum(-1, dtype=torch.int32)


def get_volume(orderside: torch.Tensor) -> torch.Tensor:
    """JaxOrderBookArrays.py:919-930."""
    return torch.where(orderside[..., 0] != cst.EMPTY_SLOT, orderside[..., 1], 0).sum(-1, dtype=torch.int32)


def get_best_ask(cfg: JAXLOB_Configuration, asks: torch.Tensor) -> torch.Tensor:
    """JaxOrderBookArrays.py:932-941: the lowest price with -1 read as maxint; -1 on an empty side."""
    p = asks[..., 0]
    mn = torch.where(p == -1, cfg.maxint, p).amin(-1)
    return torch.where(mn == cfg.maxint, -1, mn)


def get_best_bid(cfg: JAXLOB_Configuration, bids: torch.Tensor) -> torch.Tensor:
    """JaxOrderBookArrays.py:943-951: the plain maximum."""
    return bids[..., 0].amax(-1)


def get_best_bid_and_ask_inclQuants(cfg: JAXLOB_Configuration, asks: torch.Tensor, bids: torch.Tensor):
    """JaxOrderBookArrays.py:967-984: ([ask_p, ask_q], [bid_p, bid_q])."""
    ba, bb = get_best_ask(cfg, asks), get_best_bid(cfg, bids)
    qa = get_volume_at_price(asks, ba.unsqueeze(-1))
    qb = get_volume_at_price(bids, bb.unsqueeze(-1))
    return torch.stack((ba, qa), -1).to(torch.int32), torch.stack((bb, qb), -1).to(torch.int32)


def get_order_ids(orderside: torch.Tensor) -> torch.Tensor:
    """JaxOrderBookArrays.py:1200-1209: jnp.unique(ids, size=nO, fill_value=1): ascending unique
    order ids, padded with 1."""
    s, _ = torch.sort(orderside[..., 2], dim=-1)
    first = torch.ones_like(s, dtype=torch.bool)
    first[..., 1:] = s[..., 1:] != s[..., :-1]
    rank = first.to(torch.int64).cumsum(-1) - 1          # equal ids share a rank (and a value)
    return torch.ones_like(s).scatter_(-1, rank, s)


def _first_row(orderside: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """The first row where m holds, or six NEGATIVE_RETURN_ID."""
    idx = m.to(torch.int32).argmax(-1, keepdim=True)     # (the first maximum)
    row = torch.gather(orderside, -2, idx.unsqueeze(-1).expand(idx.shape + (orderside.shape[-1],))).squeeze(-2)
    return torch.where(m.any(-1, keepdim=True), row, cst.NEGATIVE_RETURN_ID).to(torch.int32)


def get_order_by_id(orderside: torch.Tensor, order_id) -> torch.Tensor:
    """JaxOrderBookArrays.py:1048-1071."""
    return _first_row(orderside, orderside[..., 2] == order_id)


def get_order_by_tid(orderside: torch.Tensor, trade_id) -> torch.Tensor:
    """JaxOrderBookArrays.py:1074-1097."""
    return _first_row(orderside, orderside[..., 3] == trade_id)


def get_order_by_id_and_price(orderside: torch.Tensor, order_id, price) -> torch.Tensor:
    """JaxOrderBookArrays.py:1099-1124."""
    return _first_row(orderside, (orderside[..., 2] == order_id) & (orderside[..., 0] == price))


def get_order_by_time(orderside: torch.Tensor, time_s, time_ns) -> torch.Tensor:
    """JaxOrderBookArrays.py:1127-1154."""
    return _first_row(orderside, (orderside[..., 4] == time_s) & (orderside[..., 5] == time_ns))


def get_order_by_time_and_price(orderside: torch.Tensor, time_s, time_ns, price) -> torch.Tensor:
    """JaxOrderBookArrays.py:1156-1198: the first row at the time and price; if there is none, the
    first row at the time."""
    at_time = (orderside[..., 4] == time_s) & (orderside[..., 5] == time_ns)
    both = at_time & (orderside[..., 0] == price)
    return _first_row(orderside, torch.where(both.any(-1, keepdim=True), both, at_time))


def get_next_executable_order(cfg: JAXLOB_Configuration, side: int, orderside: torch.Tensor) -> torch.Tensor:
    """JaxOrderBookArrays.py:1211-1229 with _get_top_{ask,bid}_order_idx :241-268: the best-priced
    row, ties by time s, then ns, then first index.  Only the ask side reads -1 prices as maxint,
    and it compares the raw price column with that minimum."""
    p = orderside[..., 0]
    if side == 0:
        best = torch.where(p == -1, cfg.maxint, p).amin(-1, keepdim=True)
    elif side == 1:
        best = p.amax(-1, keepdim=True)
    else:
        raise ValueError('Side must be 0 or 1')
    times = torch.where(p == best, orderside[..., 4], cfg.maxint)
    times_ns = torch.where(times == times.amin(-1, keepdim=True), orderside[..., 5], cfg.maxint)
    idx = (times_ns == times_ns.amin(-1, keepdim=True)).to(torch.int32).argmax(-1, keepdim=True)
    return torch.gather(orderside, -2, idx.unsqueeze(-1).expand(idx.shape + (orderside.shape[-1],))).squeeze(-2)


# ------------------------------------------------------------------------------- the wrapper
class OrderBook:
    """jorderbook.OrderBook (jorderbook.py:25-268)."""

    def __init__(self, cfg: Optional[JAXLOB_Configuration] = None, prng_partitionable: bool = True,
                 device=None) -> None:
        self.cfg = cfg if cfg is not None else JAXLOB_Configuration()
        self.prng_partitionable = prng_partitionable
        self.device = torch.device("cuda" if device is None else device)

    # -- states
    def init(self, n_env: Optional[int] = None) -> LobState:
        """jorderbook.py:32-38: empty sides and trade log, key PRNGKey(cfg.seed) = [0, seed]."""
        asks = engine.init_orderside(self.cfg.nOrders, n_env, self.device)
        bids = engine.init_orderside(self.cfg.nOrders, n_env, self.device)
        trades = engine.init_trades(self.cfg.nTrades, n_env, self.device)
        seed = self.cfg.seed & 0xFFFFFFFF
        key = torch.tensor([0, seed - (1 << 32) if seed >= (1 << 31) else seed], dtype=torch.int32, device=self.device)
        if n_env is not None:
            key = key.expand(n_env, 2).contiguous()
        return LobState(asks, bids, trades, key)

    def reset(self, l2_book=None, time=None, n_env: Optional[int] = None) -> LobState:
        """jorderbook.py:40-53: an empty book, or the book of an L2 snapshot ([4 * levels] or
        [E, 4 * levels]) rebuilt from init_msgs_from_l2 at `time` (default [0, 0])."""
        if l2_book is not None:
            l2 = torch.as_tensor(l2_book, device=self.device)
            if l2.dim() == 2:
                if n_env is not None and n_env != l2.shape[0]:
                    raise ValueError(f"l2_book has {l2.shape[0]} rows, n_env is {n_env}")
                n_env = l2.shape[0]
        state = self.init(n_env)
        if l2_book is not None:
            msgs = init_msgs_from_l2(self.cfg, l2, time=[0, 0] if time is None else time, device=self.device)
            state = self.process_orders_array(state, msgs)
        return state

    # -- processing
    def _split(self, key: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """key, sub = jax.random.split(key), per env row."""
        from .env import split_keys
        if key.dtype != torch.int32 or key.shape[-1] != 2 or key.dim() not in (1, 2):
            raise ValueError(f"key must be int32 [2] or [E, 2], got {key.dtype} {tuple(key.shape)}")
        ks = split_keys(key.reshape(-1, 2), 2, self.prng_partitionable)
        if key.dim() == 1:
            return ks[0, 0], ks[0, 1]
        return ks[:, 0].contiguous(), ks[:, 1].contiguous()

    def _scan(self, state: LobState, msgs: torch.Tensor, n_levels: Optional[int]):
        asks, bids, trades, key = state
        if not (asks.is_cuda and key.is_cuda):  # (no host fall-back: the queries run anywhere, the engine does not)
            raise RuntimeError("hftlob kernels need device (HIP) tensors; the state is on the CPU")
        single = asks.dim() == 2
        a, b, t = (engine._batched(x, 2).clone().contiguous() for x in (asks, bids, trades))
        E = a.shape[0]
        msgs = torch.as_tensor(msgs, device=a.device).to(torch.int32)
        if msgs.dim() == 2:
            msgs = msgs.unsqueeze(0).expand(E, -1, -1)
        if msgs.dim() != 3 or msgs.shape[0] != E or msgs.shape[2] != 8:
            raise ValueError(f"msgs must be [M, 8] or [{E}, M, 8], got {tuple(msgs.shape)}")
        msgs = msgs.contiguous()
        M = msgs.shape[1]
        key, sub = self._split(key)
        keys = sub.reshape(-1, 2).expand(E, 2).contiguous()
        depth = None
        if n_levels is None:
            engine.book_process_(self.cfg, msgs, a, b, t, keys=keys, prng_partitionable=self.prng_partitionable)
        else:
            depth = torch.empty((E, M, n_levels, 4), dtype=torch.int32, device=a.device)
            if M > 0:
                engine.book_process_depth_(self.cfg, msgs, a, b, t, n_levels, M, depth, keys=keys,
                                           prng_partitionable=self.prng_partitionable)
            elif not 1 <= n_levels <= engine.MAX_DEPTH_LEVELS:
                raise ValueError(f"n_levels must be in 1..{engine.MAX_DEPTH_LEVELS}, got {n_levels}")
            depth = depth.reshape(E, M, 4 * n_levels)
        if single:
            a, b, t = a[0], b[0], t[0]
            depth = depth[0] if depth is not None else None
        return LobState(a, b, t, key), depth

    def process_order(self, state: LobState, quote: Dict, from_data: bool = False, verbose: bool = False) -> LobState:
        """jorderbook.py:55-95: a quote dict (see quote_to_msg) as one message."""
        return self.process_order_array(state, torch.tensor(quote_to_msg(quote), dtype=torch.int32, device=state.asks.device))

    def process_order_array(self, state: LobState, quote, from_data: bool = False, verbose: bool = False) -> LobState:
        """jorderbook.py:97-109: one message row [8] (or one per env, [E, 8])."""
        q = torch.as_tensor(quote, device=state.asks.device)
        return self._scan(state, q.unsqueeze(-2), None)[0]

    def process_orders_array(self, state: LobState, msgs) -> LobState:
        """jorderbook.py:111-120: the messages [M, 8] (or [E, M, 8]) in sequence."""
        return self._scan(state, msgs, None)[0]

    def process_orders_array_l2(self, state: LobState, msgs, n_levels: int) -> Tuple[LobState, torch.Tensor]:
        """jorderbook.py:122-135: the messages in sequence and get_L2_state after each one:
        (state, l2_states [M, 4 * n_levels]) ([E, M, 4 * n_levels] batched), in one launch."""
        return self._scan(state, msgs, int(n_levels))

    # -- queries
    def get_volume_at_price(self, state: LobState, side: int, price, init_only: bool = False) -> torch.Tensor:
        """jorderbook.py:137-156."""
        s = _side(state, side)
        p = price.unsqueeze(-1) if torch.is_tensor(price) and price.dim() > 0 else price  # (one price per env)
        return get_init_volume_at_price(s, p, self.cfg) if init_only else get_volume_at_price(s, p)

    def get_volume(self, state: LobState, side: int) -> torch.Tensor:
        return get_volume(_side(state, side))

    def get_best_price(self, state: LobState, side: int) -> torch.Tensor:
        """jorderbook.py:158-169: side 1 the best bid, else the best ask."""
        _side(state, side)
        return self.get_best_bid(state) if side == 1 else self.get_best_ask(state)

    def get_best_bid(self, state: LobState) -> torch.Tensor:
        return get_best_bid(self.cfg, state.bids)

    def get_best_ask(self, state: LobState) -> torch.Tensor:
        return get_best_ask(self.cfg, state.asks)

    def get_best_bid_and_ask_inclQuants(self, state: LobState) -> Tuple[torch.Tensor, torch.Tensor]:
        return get_best_bid_and_ask_inclQuants(self.cfg, state.asks, state.bids)

    def get_L2_state(self, state: LobState, n_levels: int) -> torch.Tensor:
        """jorderbook.py:192-198, by the hftlob_book_depth kernel."""
        return engine.get_L2_state(state.asks, state.bids, n_levels, self.cfg)

    def get_side_ids(self, state: LobState, side: int) -> torch.Tensor:
        """jorderbook.py:200-212."""
        return get_order_ids(_side(state, side))

    def get_order(self, state: LobState, side: int, order_id, price=None) -> torch.Tensor:
        """jorderbook.py:214-232."""
        s = _side(state, side)
        return get_order_by_id(s, order_id) if price is None else get_order_by_id_and_price(s, order_id, price)

    def get_order_by_tid(self, state: LobState, side: int, trade_id) -> torch.Tensor:
        return get_order_by_tid(_side(state, side), trade_id)

    def get_order_at_time(self, state: LobState, side: int, time_s, time_ns, price=None) -> torch.Tensor:
        """jorderbook.py:234-253."""
        s = _side(state, side)
        if price is None:
            return get_order_by_time(s, time_s, time_ns)
        return get_order_by_time_and_price(s, time_s, time_ns, price)

    def get_next_executable_order(self, state: LobState, side: int) -> torch.Tensor:
        """jorderbook.py:256-268."""
        return get_next_executable_order(self.cfg, side, _side(state, side))
