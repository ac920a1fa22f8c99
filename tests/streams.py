"""Seeded random message streams that exercise the engine's quirks (test helper)."""
import numpy as np


def random_streams(n_env, n_msg, seed, price0=1000, tick=1, spread=12, init_frac=0.1, garbage=0.02, nO=100):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n_env, n_msg, 8), dtype=np.int32)
    for e in range(n_env):
        live = []                       # (oid, side, price)
        next_oid = 1000
        t, tn = 34200, 0
        for k in range(n_msg):
            if rng.random() < 0.8:
                tn += int(rng.integers(1, 1000))
            if rng.random() < 0.05:
                t += 1
            u = rng.random()
            side = int(rng.choice([-1, 1]))
            price = price0 + side * int(rng.integers(-3, spread)) * tick
            qty = int(rng.integers(1, 60))
            if rng.random() < 0.01:
                qty = int(rng.integers(-3, 1))
            tid = int(rng.integers(1, 6))
            if u < 0.45:
                typ, oid = 1, next_oid
                next_oid += 1
                live.append((oid, side, price))
            elif u < 0.72:
                typ = int(rng.choice([2, 3]))
                if live and rng.random() < 0.75:
                    oid, side, price = live[int(rng.integers(0, len(live)))]
                elif rng.random() < init_frac * 5:
                    oid = -2 - int(rng.integers(0, 3))      # init-id fallback path
                else:
                    oid = int(rng.integers(1, 5000))
            elif u < 0.95:
                typ = 4
                oid = live[int(rng.integers(0, len(live)))][0] if live else 7
            elif u < 1.0 - garbage:
                typ, side, qty, price, oid = 0, 0, 0, 0, 0
            else:
                typ = int(rng.choice([0, 5, 6, 7])); side = int(rng.choice([-1, 0, 1])); oid = 9
            out[e, k] = (typ, side, qty, price, oid, tid, t, tn)
    return out


def init_book_messages(n_env, seed, price0=1000, tick=1, depth=10):
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.zeros((n_env, 2 * depth, 8), dtype=np.int32)
    for e in range(n_env):
        for k in range(2 * depth):
            lvl = k // 2 + 1
            side = -1 if k % 2 == 0 else 1
            q = int(rng.integers(0, 200)) if rng.random() > 0.1 else 0
            m[e, k] = (1, side, q, price0 - side * lvl * tick + (5 if side == -1 else -5), -2, -2 - k, 34199, 0)
    return m


def top_streams(n_env, n_msg, seed, price0=1000, maxint=2**31 - 1):
    """Streams for the top-of-book slot (_get_top_*_order_idx) and time priority: a narrow
    price band so most orders join or cross the best level, times drawn from a small set (ties on
    (ts, tns) and orders EARLIER than the standing top are common, so the slot tie-break and the
    time-priority replacement both run), partial and full fills, cancels at the best price, and a
    few maxint times."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n_env, n_msg, 8), dtype=np.int32)
    for e in range(n_env):
        live = []
        next_oid = 5000
        for k in range(n_msg):
            t = 34200 + int(rng.integers(0, 3))
            tn = int(rng.integers(0, 4)) * 100
            if rng.random() < 0.01:
                t = maxint
            if rng.random() < 0.01:
                tn = maxint
            side = int(rng.choice([-1, 1]))
            price = price0 + side * int(rng.integers(-2, 3))
            qty = int(rng.integers(1, 40))
            tid = int(rng.integers(1, 4))
            u = rng.random()
            if u < 0.5:
                typ, oid = 1, next_oid
                next_oid += 1
                live.append((oid, side, price))
            elif u < 0.7 and live:
                typ = int(rng.choice([2, 3]))
                oid, side, price = live[int(rng.integers(0, len(live)))]
            elif u < 0.9:
                typ = 4
                oid = live[int(rng.integers(0, len(live)))][0] if live else 7
            else:                                   # marketable limit: crosses deep
                typ, oid = 1, next_oid
                next_oid += 1
                price = price0 - side * 5
            out[e, k] = (typ, side, qty, price, oid, tid, t, tn)
    return out


def neg1_trade_streams(n_env, n_msg, seed, price0=1000):
    """top_streams whose crossing messages (type 4 and the deep marketable limits) often carry
    oid == -1 or time == -1.  match_order (JaxOrderBookArrays.py:205) writes a trade into the
    first row whose col 4 (the message TIME, TradesFeat.SEC) is -1, so a trade made by a
    time == -1 message leaves its row free for the next trade, while an oid == -1 one does not."""
    out = top_streams(n_env, n_msg, seed, price0)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    crossing = (out[..., 0] == 4) | ((out[..., 0] == 1) & (np.abs(out[..., 3] - price0) == 5))
    u = rng.random(out.shape[:2])
    out[..., 4] = np.where(crossing & (u < 0.3), -1, out[..., 4])
    out[..., 6] = np.where(crossing & (u >= 0.3) & (u < 0.6), -1, out[..., 6])
    out[..., 7] = np.where(crossing & (u >= 0.5) & (u < 0.6), -1, out[..., 7])
    return out


def full_book_messages(n_env, seed, nO=100, lo=0.85, hi=1.0, price0=1000, init_id=-2):
    """Init messages that leave each side holding between lo * nO and hi * nO orders (per env and
    side), at distinct prices behind the touch, a third of them with the init id (-2, the
    get_init_id_match candidates): books whose last slot is occupied or not, and a few free rows,
    for the no-op skip's room test.  (nO = 1: a side holds one order or none.)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for e in range(n_env):
        r = []
        for side in (-1, 1):
            n = int(rng.integers(int(lo * nO), int(hi * nO) + 1))
            for k in range(n):
                price = price0 - side * (3 + k) + (0 if side == 1 else 0)
                oid = init_id if rng.random() < 0.33 else 100000 + 1000 * (side + 1) + k
                r.append((1, side, int(rng.integers(1, 50)), price, oid, -2 - k, 34199, k))
        rows.append(r)
    m = max(len(r) for r in rows)
    out = np.zeros((n_env, m, 8), dtype=np.int32)  # doNothing padding
    for e, r in enumerate(rows):
        if r:
            out[e, :len(r)] = r
    return out


def noop_streams(n_env, n_msg, seed, price0=1000, nO=100):
    """Streams for the chunk pre-pass that skips messages which leave the book unchanged
    (hftlob.hip chunk_noops): mostly cancels of ids no row holds (the replayed day's common
    cancel: its -1 index wraps to the last slot), at prices that do and do not hold init-id rows,
    with quantities 1..50, 0, -1 (skippable) and below -1 (which end the skipping); doNothing rows;
    cancels of live ids and of id -1; non-crossing adds that fill the last free rows of a side
    (the room test's boundary), adds of no quantity (into sides with and without a free row),
    adds carrying an init id or a -1 field (which end the skipping), and executions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n_env, n_msg, 8), dtype=np.int32)
    for e in range(n_env):
        live = []
        next_oid = 20000
        t, tn = 34200, 0
        for k in range(n_msg):
            tn += int(rng.integers(1, 500))
            side = int(rng.choice([-1, 1]))
            lvl = int(rng.integers(1, 12))
            price = price0 - side * lvl
            qty = int(rng.integers(1, 50))
            tid = int(rng.integers(1, 6))
            u = rng.random()
            if u < 0.25:                      # non-crossing add (a fifth of no quantity: a full side evicts for them)
                typ, oid = 1, next_oid
                next_oid += 1
                if rng.random() < 0.2:
                    qty = int(rng.choice([0, 0, -1, -4]))
                else:
                    live.append((oid, side, price))
            elif u < 0.62:                    # cancel of an id no row holds
                typ = int(rng.choice([2, 3]))
                oid = int(rng.integers(1, 10**6))
                v = rng.random()
                qty = 0 if v < 0.08 else (-1 if v < 0.14 else qty)
            elif u < 0.70 and live:           # cancel of a live id
                typ = int(rng.choice([2, 3]))
                oid, side, price = live[int(rng.integers(0, len(live)))]
            elif u < 0.75:                    # zero-quantity cancel
                typ, oid, qty = 3, int(rng.integers(1, 10**6)), 0
            elif u < 0.80:                    # doNothing row
                typ, side, qty, price, oid, tid = 0, 0, 0, 0, 0, 0
            elif u < 0.82:                    # cancel of id -1
                typ, oid = int(rng.choice([2, 3])), -1
                qty = int(rng.choice([1, 0, -1]))
            elif u < 0.85:                    # init-id cancel (get_init_id_match candidates)
                typ, oid = 2, -2 - int(rng.integers(0, 25))
            elif u < 0.87:                    # add carrying an init id (ends the skipping)
                typ, oid = 1, -2 - int(rng.integers(0, 21))
            elif u < 0.89:                    # add with a -1 field (ends the FAST variant)
                typ, oid, tid = 1, next_oid, -1
                next_oid += 1
            elif u < 0.90:                    # cancel of a negative quantity (ends the skipping)
                typ, oid, qty = int(rng.choice([2, 3])), int(rng.integers(1, 10**6)), -int(rng.integers(2, 6))
            elif u < 0.95:                    # execution
                typ = 4
                oid = live[int(rng.integers(0, len(live)))][0] if live else 7
            else:                             # marketable limit (sometimes of no quantity: it matches nothing)
                typ, oid = 1, next_oid
                next_oid += 1
                price = price0 + side * 4
                if rng.random() < 0.2:
                    qty = 0
            out[e, k] = (typ, side, qty, price, oid, tid, t, tn)
    return out


def odd_add_streams(n_env, n_msg, seed, price0=1000, maxint=2**31 - 1):
    """random_streams whose adds include the kernel's RARE decode cases (hftlob.hip decode_msgs):
    limit and type-4 messages priced at or below 0 (-1, -2, -7: a negative ask crosses every bid,
    a negative bid rests behind them all), priced maxint, and add-kind messages whose side is not
    -1 / 1 (type 1 with side 0 or 2 is an ask_lim with that side, as cond_type_side sends it;
    type 4 with side 0 / 2 flips to 0 / -2).  The common add handlers assume 0 <= price, qty > 0
    and side -1 / 1; these must take the general path and leave the book exactly as the oracle's."""
    out = random_streams(n_env, n_msg, seed, price0=price0)
    rng = np.random.Generator(np.random.PCG64(seed + 7))
    add = (out[..., 0] == 1) | (out[..., 0] == 4)
    u = rng.random(out.shape[:2])
    neg = add & (u < 0.06)
    out[..., 3] = np.where(neg, rng.choice([-1, -2, -7, 0], size=out.shape[:2]), out[..., 3])
    top = add & (u >= 0.06) & (u < 0.08)
    out[..., 3] = np.where(top, maxint, out[..., 3])
    odd = add & (u >= 0.08) & (u < 0.13)
    out[..., 1] = np.where(odd, rng.choice([0, 2, -2], size=out.shape[:2]), out[..., 1])
    return out


def filter_carry_streams(n_env, seed, price0=1000, n_chunks=4):
    """Streams for the no-op filter carried from one chunk to the next (hftlob.hip chunk_noops:
    filt_ok; built at the first chunk from the book's ids and init-id rows, then only each chunk's
    add ids go in while no chunk holds a brk message).  Chunk 0 has no brk message; from chunk 1 on,
    adds with new ids and (in half of the envs) adds carrying an init id fall in a later chunk than
    the first, and the following chunks cancel them: by id (quantities 1..50 and -1, which the
    pre-pass would skip if the filter missed the id), and by an unknown id at an init-id add's price
    (a get_init_id_match candidate the filter must hold), among cancels of ids no row holds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = 64 * n_chunks
    out = np.zeros((n_env, M, 8), dtype=np.int32)
    for e in range(n_env):
        added, init_px = [], []
        next_oid, t, tn = 30000, 34200, 0
        brk_env = rng.random() < 0.5
        for k in range(M):
            ch = k // 64
            tn += int(rng.integers(1, 500))
            side = int(rng.choice([-1, 1]))
            price = price0 - side * int(rng.integers(1, 12))
            qty = int(rng.integers(1, 50))
            tid = int(rng.integers(1, 6))
            u = rng.random()
            if ch >= 1 and brk_env and u < 0.05:       # add carrying an init id (brk) in a later chunk
                typ, oid = 1, -2 - int(rng.integers(0, 21))
                init_px.append((side, price))
            elif u < 0.30:                              # non-crossing add with a new id
                typ, oid = 1, next_oid
                next_oid += 1
                added.append((oid, side, price))
            elif ch >= 1 and u < 0.60 and added:        # cancel of an id an earlier message added
                typ = 2
                oid, side, price = added[int(rng.integers(0, len(added)))]
                qty = -1 if rng.random() < 0.15 else qty
            elif ch >= 1 and u < 0.70 and init_px:      # unknown id at an init-id add's price
                typ, oid = 2, int(rng.integers(10**6, 2 * 10**6))
                side, price = init_px[int(rng.integers(0, len(init_px)))]
            elif u < 0.90:                              # cancel of an id no row holds
                typ, oid = int(rng.choice([2, 3])), int(rng.integers(10**6, 2 * 10**6))
            else:                                       # doNothing row
                typ, side, qty, price, oid, tid = 0, 0, 0, 0, 0, 0
            out[e, k] = (typ, side, qty, price, oid, tid, t, tn)
    return out


def miss_empty_streams(n_env, seed, price0=1000, n_chunks=4, nO=100):
    """Streams for the cancels chunk_noops marks H_MISS (no row holds the id, no init-id row at the
    price: the -1 index wraps to the last slot) whose side's last slot is empty when they run
    although the pre-pass could not prove it (hftlob.hip cancel: the early return on p == -1).
    Over full_book_messages books (90-99 % full), each chunk cancels a few of the init book's orders
    by id on one side (freeing rows), then adds to that side more orders than it had free rows
    below the last slot, then cancels unknown ids beyond the init prices (quantities 1..20 and -1).
    In half of the envs chunk 1 and the last chunk also cancel an unknown id with a quantity below
    -1 first: wrapping to an empty last slot it leaves q > 0 at p == -1 (the side's PM1: the book
    leaves the FAST variant); chunk 1's other cancels go to the other side, so chunk 2's wrapping
    cancels (marked H_MISS, the book FAST again only if the flag were lost) meet that row; in the last
    chunk only one (of quantity 1) does, so the row is still there at the end."""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = 64 * n_chunks
    out = np.zeros((n_env, M, 8), dtype=np.int32)
    for e in range(n_env):
        hole_env = rng.random() < 0.5
        next_oid, t, tn, k = 50000, 34200, 0, 0
        cancelled = set()
        for ch in range(n_chunks):
            side = int(rng.choice([-1, 1]))
            row = []
            for _ in range(int(rng.integers(0, 5))):  # cancels of init-book orders by id (known ids)
                j = int(rng.integers(0, int(0.9 * nO)))
                oid = 100000 + 1000 * (side + 1) + j
                if oid not in cancelled:
                    cancelled.add(oid)
                    row.append((2 if side == -1 else 3, side, 50, price0 - side * (3 + j), oid))
            hole = hole_env and (ch == 1 or ch == n_chunks - 1)
            if hole:  # an unknown id, quantity below -1: q = -1 - qty > 0 stays at p == -1
                row.append((2 if side == -1 else 3, side, -int(rng.integers(3, 7)), price0 - side * (nO + 9),
                            int(rng.integers(10**6, 2 * 10**6))))
            for _ in range(int(rng.integers(3, 9))):  # non-crossing adds to the side
                row.append((1, side, int(rng.integers(1, 40)), price0 - side * int(rng.integers(3, 12)), next_oid))
                next_oid += 1
            if hole and ch == n_chunks - 1:  # one wrapping cancel of 1 meets the row, which stays to the end
                row.append((2 if side == -1 else 3, side, 1, price0 - side * (nO + 5), int(rng.integers(10**6, 2 * 10**6))))
                while len(row) < 64:
                    row.append((0, 0, 0, 0, 0))
            while len(row) < 64:  # wrapping cancels of unknown ids beyond the init prices
                q = -1 if rng.random() < 0.1 else int(rng.integers(1, 21))
                # (after chunk 1's hole: the other side only, so the row reaches chunk 2, where the
                # wrapping cancels are H_MISS again and meet it)
                sd = -side if hole else (side if rng.random() < 0.8 else -side)
                row.append((2 if sd == -1 else 3, sd, q, price0 - sd * (nO + 5 + int(rng.integers(0, 4))),
                            int(rng.integers(10**6, 2 * 10**6))))
            for typ, sd, q, price, oid in row[:64]:
                tn += int(rng.integers(1, 500))
                out[e, k] = (typ, sd, q, price, oid, int(rng.integers(1, 6)), t, tn)
                k += 1
    return out


def prefilled_trades(n_env, nT, seed, rows=None, price0=1000):
    """Incoming trade logs whose first `rows` rows (default nT - 2, at least 0) hold earlier trades
    (col 4, the trade's TIME, is not -1) and whose other rows are free (-1): the next trades go to
    rows nT - 2 and nT - 1, and every later one overwrites the last row (match_order's -1 index)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = max(0, nT - 2) if rows is None else rows
    t = np.full((n_env, nT, 8), -1, np.int32)
    t[:, :n, 0] = price0 + rng.integers(-3, 4, (n_env, n))
    t[:, :n, 1] = rng.integers(1, 40, (n_env, n)) * rng.choice([-1, 1], (n_env, n))
    t[:, :n, 2] = rng.integers(1000, 5000, (n_env, n))
    t[:, :n, 3] = rng.integers(1000, 5000, (n_env, n))
    t[:, :n, 4] = 34100 + np.arange(n)[None, :]
    t[:, :n, 5] = rng.integers(0, 10**9, (n_env, n))
    t[:, :n, 6] = rng.integers(1, 6, (n_env, n))
    t[:, :n, 7] = rng.integers(1, 6, (n_env, n))
    return t


def init_range_streams(n_env, n_msg, seed, init_id=-2, price0=1000, nO=100):
    """noop_streams with a sixth of the messages replaced by the two halves of get_init_id_match's
    id range test [init_id - 2 * book_depth, init_id]: non-crossing adds carrying an id in
    [init_id - 20, init_id - 7] (init-id rows at book_depth 10, ordinary rows at book_depth 3 and 0)
    or init_id itself, and, later, cancels of ids no row holds at those adds' prices with a quantity
    of at most the add's (at depth 10 they take the init-id row; at depth 3 only init_id's rows,
    else the -1 index wraps to the last slot), and cancels by those ids themselves."""
    out = noop_streams(n_env, n_msg, seed, price0=price0, nO=nO)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    for e in range(n_env):
        rows = []                                   # (side, price, qty, oid)
        for k in range(n_msg):
            u = rng.random()
            if u >= 1 / 6:
                continue
            typ0, sd0, q0, p0, o0, tid, t, tn = (int(x) for x in out[e, k])
            if u < 0.07 or not rows:
                side = int(rng.choice([-1, 1]))
                price = price0 - side * int(rng.integers(1, 12))
                qty = int(rng.integers(5, 50))
                oid = init_id if rng.random() < 0.2 else init_id - int(rng.integers(7, 21))
                rows.append((side, price, qty, oid))
                out[e, k] = (1, side, qty, price, oid, max(tid, 1), t, tn)
            else:
                side, price, qty, oid = rows[int(rng.integers(0, len(rows)))]
                if rng.random() < 0.25:             # by the id itself
                    out[e, k] = (2, side, int(rng.integers(1, qty + 1)), price, oid, max(tid, 1), t, tn)
                else:                               # an id no row holds, at the init-id add's price
                    out[e, k] = (int(rng.choice([2, 3])), side, int(rng.integers(1, qty + 1)), price,
                                 int(rng.integers(10**6, 2 * 10**6)), max(tid, 1), t, tn)
    return out


EXTREME_VALUES = (-2**31, -2**31 + 1, 2**31 - 2, 2**31 - 1, 0, -1, -2, -22, -23)


def extreme_field_streams(n_env, n_msg, seed, p=0.12, price0=1000):
    """random_streams whose order ids, prices, seconds and nanoseconds are replaced, each with
    probability p and independently, by int32's extremes and the engine's special values
    (EXTREME_VALUES: INT32_MIN and its neighbour, INT32_MAX and its neighbour, 0, -1 = the empty
    marker, -2 = the init id, -22 / -23 = the ends of its range at book_depth 10): the decode
    classifies on sign, the no-op filter hashes ids and prices, the top-of-book slot compares times.
    A tenth of the positive quantities become 2^20 .. 2^22, so that 256 slots sum below 2^30 and
    every quantity sum and difference stays inside int32 (beyond it the oracles have no answer)."""
    out = random_streams(n_env, n_msg, seed, price0=price0)
    rng = np.random.Generator(np.random.PCG64(seed + 13))
    shp = out.shape[:2]
    vals = np.array(EXTREME_VALUES, dtype=np.int64)
    for col in (4, 3, 6, 7):
        hit = rng.random(shp) < p
        out[..., col] = np.where(hit, rng.choice(vals, size=shp), out[..., col]).astype(np.int32)
    big = (rng.random(shp) < 0.1) & (out[..., 2] > 0)
    out[..., 2] = np.where(big, rng.integers(2**20, 2**22 + 1, shp), out[..., 2]).astype(np.int32)
    return out
