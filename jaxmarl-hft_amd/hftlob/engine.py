"""Order-book engine operators (device tensors in, device tensors out).

Mirrors the reference operator API of ``gymnax_exchange/jaxob/
JaxOrderBookArrays.py`` for the batched case the MARL path uses:

* ``scan_through_entire_array_save_bidask(cfg, key, msg_array, book_state,
  N_steps)`` (:791-823) -> ``((asks, bids, trades), (best_asks[-N:],
  best_bids[-N:]))``
* ``scan_through_entire_array(cfg, key, msg_array, book_state)`` (:736-756)
* ``scan_through_entire_array_save_states(cfg, key, msg_array, book_state,
  N_steps)`` (:758-789) -> ``(all_asks[-N:], all_bids[-N:], trades)``
* ``get_L2_state(asks, bids, n_levels, cfg)`` (:1231-1264)

Every array carries a leading env dimension (the reference is vmapped; here
the batch is explicit).  ``key`` (uint32 words, shape (2,) shared by every
env or (E, 2) per env; None = PRNGKey(0)) only matters for cancel modes 2/3,
where message k of env e draws from split(key_e, M)[k] (:753,784,816).
Functional like the reference: inputs are not modified.  ``book_process_`` is
the in-place form, ``book_process_depth_`` the in-place scan that also writes
the L2 view and / or the sides after each of the last ``n_keep`` messages.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from .config import JAXLOB_Configuration
from .layout import pack_lob_cfg


def _lob(cfg: JAXLOB_Configuration, prng_partitionable: bool = True):
    return pack_lob_cfg(cfg, prng_partitionable)


def _keys(key, E: int, device) -> torch.Tensor:
    """The scan key per env as int32 [E, 2] (uint32 bit patterns)."""
    if key is None:
        return torch.zeros((E, 2), dtype=torch.int32, device=device)
    k = torch.as_tensor(key, device=device)
    if k.dtype != torch.int32:
        k = k.to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int64)
        k = torch.where(k >= 2**31, k - 2**32, k).to(torch.int32)
    if k.shape == (2,):
        k = k.expand(E, 2)
    if tuple(k.shape) != (E, 2):
        raise ValueError(f"key must have shape (2,) or ({E}, 2), got {tuple(k.shape)}")
    return k.contiguous()


def _batched(x: torch.Tensor, tail: int) -> torch.Tensor:
    return x if x.dim() == tail + 1 else x.unsqueeze(0)


def book_process_(cfg: JAXLOB_Configuration, msgs: torch.Tensor, asks: torch.Tensor, bids: torch.Tensor,
                  trades: torch.Tensor, best_asks: Optional[torch.Tensor] = None,
                  best_bids: Optional[torch.Tensor] = None, stream=None, keys: Optional[torch.Tensor] = None,
                  prng_partitionable: bool = True) -> None:
    """In place: process msgs [E, M, 8] through (asks, bids [E, nO, 6], trades [E, nT, 8]).
    keys: int32 [E, 2] scan keys (required for cancel_mode 2/3)."""
    E, M = msgs.shape[0], msgs.shape[1]
    for t, shp in ((msgs, (E, M, 8)), (asks, (E, cfg.nOrders, 6)), (bids, (E, cfg.nOrders, 6)),
                   (trades, (E, cfg.nTrades, 8))):
        if tuple(t.shape) != shp or t.dtype != torch.int32:
            raise ValueError(f"expected int32 {shp}, got {t.dtype} {tuple(t.shape)}")
    if best_asks is not None and (tuple(best_asks.shape) != (E, M, 2) or tuple(best_bids.shape) != (E, M, 2)):
        raise ValueError("best_asks / best_bids must be int32 [E, M, 2]")
    if keys is not None and (tuple(keys.shape) != (E, 2) or keys.dtype != torch.int32):
        raise ValueError("keys must be int32 [E, 2]")
    L = _lib.lib()
    c = _lob(cfg, prng_partitionable)
    with torch.cuda.device(msgs.device):
        _lib.check(L.hftlob_book_process(C.byref(c), E, M, _lib.ptr(keys), _lib.ptr(msgs), _lib.ptr(asks),
                                         _lib.ptr(bids), _lib.ptr(trades), _lib.ptr(best_asks), _lib.ptr(best_bids),
                                         _lib.stream_ptr(stream, device=msgs.device)))


def scan_through_entire_array_save_bidask(cfg: JAXLOB_Configuration, key, msg_array: torch.Tensor,
                                          book_state: Tuple[torch.Tensor, torch.Tensor, torch.Tensor],
                                          N_steps: Optional[int] = None, prng_partitionable: bool = True):
    single = msg_array.dim() == 2
    msgs = _batched(msg_array, 2).contiguous()
    asks, bids, trades = (_batched(x, 2).clone().contiguous() for x in book_state)
    E, M = msgs.shape[0], msgs.shape[1]
    ba = torch.empty((E, M, 2), dtype=torch.int32, device=msgs.device)
    bb = torch.empty_like(ba)
    book_process_(cfg, msgs, asks, bids, trades, ba, bb, keys=_keys(key, E, msgs.device),
                  prng_partitionable=prng_partitionable)
    n = M if N_steps is None else N_steps
    ba, bb = ba[:, M - n:], bb[:, M - n:]
    if single:
        asks, bids, trades, ba, bb = asks[0], bids[0], trades[0], ba[0], bb[0]
    return (asks, bids, trades), (ba, bb)


def scan_through_entire_array(cfg: JAXLOB_Configuration, key, msg_array: torch.Tensor,
                              book_state: Tuple[torch.Tensor, torch.Tensor, torch.Tensor],
                              prng_partitionable: bool = True):
    single = msg_array.dim() == 2
    msgs = _batched(msg_array, 2).contiguous()
    asks, bids, trades = (_batched(x, 2).clone().contiguous() for x in book_state)
    book_process_(cfg, msgs, asks, bids, trades, keys=_keys(key, msgs.shape[0], msgs.device),
                  prng_partitionable=prng_partitionable)
    if single:
        return asks[0], bids[0], trades[0]
    return asks, bids, trades


MAX_DEPTH_LEVELS = 16  # HFTLOB_MAX_DEPTH_LEVELS


def book_process_depth_(cfg: JAXLOB_Configuration, msgs: torch.Tensor, asks: torch.Tensor, bids: torch.Tensor,
                        trades: torch.Tensor, n_levels: int, n_keep: Optional[int] = None,
                        depth: Optional[torch.Tensor] = None, all_asks: Optional[torch.Tensor] = None,
                        all_bids: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None, stream=None,
                        prng_partitionable: bool = True) -> None:
    """In place: book_process_ that also writes, for each of the last n_keep messages (None = all),
    the state after it: depth int32 [E, n_keep, n_levels, 4] (get_L2_state) and / or all_asks,
    all_bids int32 [E, n_keep, nO, 6].  One launch (hftlob_book_process_depth)."""
    E, M = msgs.shape[0], msgs.shape[1]
    n_keep = M if n_keep is None else int(n_keep)
    for t, shp in ((msgs, (E, M, 8)), (asks, (E, cfg.nOrders, 6)), (bids, (E, cfg.nOrders, 6)),
                   (trades, (E, cfg.nTrades, 8))):
        if tuple(t.shape) != shp or t.dtype != torch.int32:
            raise ValueError(f"expected int32 {shp}, got {t.dtype} {tuple(t.shape)}")
    if M > 0 and not 1 <= n_keep <= M:
        raise ValueError(f"n_keep must be in 1..{M}, got {n_keep}")
    if depth is None and all_asks is None and all_bids is None:
        raise ValueError("give depth and / or all_asks, all_bids")
    if (all_asks is None) != (all_bids is None):
        raise ValueError("all_asks / all_bids: both or none")
    if depth is not None:
        if not 1 <= n_levels <= MAX_DEPTH_LEVELS:
            raise ValueError(f"n_levels must be in 1..{MAX_DEPTH_LEVELS}, got {n_levels}")
        if tuple(depth.shape) != (E, n_keep, n_levels, 4) or depth.dtype != torch.int32:
            raise ValueError(f"depth must be int32 {(E, n_keep, n_levels, 4)}, got {depth.dtype} {tuple(depth.shape)}")
    for t in (all_asks, all_bids):
        if t is not None and (tuple(t.shape) != (E, n_keep, cfg.nOrders, 6) or t.dtype != torch.int32):
            raise ValueError(f"all_asks / all_bids must be int32 {(E, n_keep, cfg.nOrders, 6)}")
    if keys is not None and (tuple(keys.shape) != (E, 2) or keys.dtype != torch.int32):
        raise ValueError("keys must be int32 [E, 2]")
    L = _lib.lib()
    if E == 0 or M == 0:  # nothing to process or to write (an empty tensor has no pointer to pass)
        return
    c = _lob(cfg, prng_partitionable)
    with torch.cuda.device(msgs.device):
        _lib.check(L.hftlob_book_process_depth(C.byref(c), E, M, _lib.ptr(keys), _lib.ptr(msgs), _lib.ptr(asks),
                                               _lib.ptr(bids), _lib.ptr(trades), int(n_levels), n_keep,
                                               _lib.ptr(depth), _lib.ptr(all_asks), _lib.ptr(all_bids),
                                               _lib.stream_ptr(stream, device=msgs.device)))


def scan_through_entire_array_save_states(cfg: JAXLOB_Configuration, key, msg_array: torch.Tensor,
                                          book_state: Tuple[torch.Tensor, torch.Tensor, torch.Tensor],
                                          N_steps: Optional[int] = None, prng_partitionable: bool = True):
    """JaxOrderBookArrays.py:758-789: (all_asks[-N:], all_bids[-N:], trades), the sides after each of
    the last N_steps messages (None = all) and the final trade log.  N_steps < 1 is refused (the
    reference's [-0:] would return every state)."""
    single = msg_array.dim() == 2
    msgs = _batched(msg_array, 2).contiguous()
    asks, bids, trades = (_batched(x, 2).clone().contiguous() for x in book_state)
    E, M = msgs.shape[0], msgs.shape[1]
    n = M if N_steps is None else int(N_steps)
    if N_steps is not None and n < 1:
        raise ValueError(f"N_steps must be >= 1, got {N_steps}")
    n = min(n, M)  # (a slice longer than the scan is the whole scan)
    aa = torch.empty((E, n, cfg.nOrders, 6), dtype=torch.int32, device=msgs.device)
    ab = torch.empty_like(aa)
    if M > 0:
        book_process_depth_(cfg, msgs, asks, bids, trades, 1, n, None, aa, ab, keys=_keys(key, E, msgs.device),
                            prng_partitionable=prng_partitionable)
    if single:
        aa, ab, trades = aa[0], ab[0], trades[0]
    return aa, ab, trades


def get_L2_state(asks: torch.Tensor, bids: torch.Tensor, n_levels: int, cfg: JAXLOB_Configuration) -> torch.Tensor:
    """get_L2_state (JaxOrderBookArrays.py:1231-1264) of books [..., nO, 6]: int32 [..., 4 * n_levels],
    flattened as the reference does: [ask_p, ask_q, bid_p, bid_q] level by level."""
    if not 1 <= n_levels <= MAX_DEPTH_LEVELS:
        raise ValueError(f"n_levels must be in 1..{MAX_DEPTH_LEVELS}, got {n_levels}")
    if asks.shape != bids.shape or tuple(asks.shape[-2:]) != (cfg.nOrders, 6) or asks.dtype != torch.int32 \
            or bids.dtype != torch.int32:
        raise ValueError(f"asks / bids must be int32 [..., {cfg.nOrders}, 6] of one shape")
    lead = tuple(asks.shape[:-2])
    a = asks.reshape(-1, cfg.nOrders, 6).contiguous()
    b = bids.reshape(-1, cfg.nOrders, 6).contiguous()
    out = torch.empty((a.shape[0], 4 * n_levels), dtype=torch.int32, device=a.device)
    c = _lob(cfg)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().hftlob_book_depth(C.byref(c), a.shape[0], int(n_levels), _lib.ptr(a), _lib.ptr(b),
                                                _lib.ptr(out), _lib.stream_ptr(None, device=a.device)))
    return out.reshape(lead + (4 * n_levels,))


def init_orderside(nOrders: int = 100, n_env: Optional[int] = None, device="cuda") -> torch.Tensor:
    """init_orderside — JaxOrderBookArrays.py:987-997 (all -1)."""
    shape = (nOrders, 6) if n_env is None else (n_env, nOrders, 6)
    return torch.full(shape, -1, dtype=torch.int32, device=device)


def init_trades(nTrades: int = 100, n_env: Optional[int] = None, device="cuda") -> torch.Tensor:
    shape = (nTrades, 8) if n_env is None else (n_env, nTrades, 8)
    return torch.full(shape, -1, dtype=torch.int32, device=device)
