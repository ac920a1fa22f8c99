"""The grouped policy step on the GPU (hftlob_policy_step_grouped, hftlob.train.policy.policy_step_grouped).
Every group of a grouped launch must equal bit for bit what the single operators give for that group alone
(hftlob_policy_step for a flat one-head group, hftlob_policy_step_multi otherwise), in both modes, whatever
the other groups and their order; the fixtures of tests/policy_cases.py are also held to their float64
reference under the project's tolerance, per tensor |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, with the
actions exact (their top-two gap of at least 1e-3 is held on the CPU by tests/test_policy_cases_cpu.py).

The shapes are the smallest at which the tile and group arithmetic can go wrong: groups of one row, of exactly
one and two tiles and of a tile plus or minus one row; groups behind one that ends inside a tile; mixed head
counts (the four-block instantiation) and one head everywhere (the one-block instantiation) at the group
limit of eight; every (FC, H) instantiation."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_cases as PC
from hftlob import _lib
from hftlob.train import policy as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("h", "action", "log_prob", "value", "logits")

# name: (FC, H, [(B, D, nvec)])
SETS = {
    "two_types": (64, 64, [(16, 2, (10,)), (16, 12, (13,))]),
    "ragged": (64, 128, [(1, 1, (1,)), (17, 61, (3, 16, 1, 5)), (33, 64, (16,)), (16, 12, (13,))]),
    "eight": (256, 256, [(B, (2, 12, 61, 64)[g % 4], ((10, 13, 16, 1)[g % 4],))
                         for g, B in enumerate((1, 15, 16, 17, 31, 32, 33, 48))]),
}


def key_of(g):
    """Group g's sample key: both words set, different per group."""
    k = np.array([0x9E3779B9 + 0x01000193 * g, 0x7F4A7C15 ^ (0x85EBCA6B * (g + 1) & 0xFFFFFFFF)], dtype=np.uint64)
    return torch.from_numpy((k & 0xFFFFFFFF).astype(np.uint32).view(np.int32).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def group_set(name):
    """The groups of a set on the device, one seed offset per group: a list of (W, x, heads), heads an int for
    a flat one-head group (hftlob_policy_step) and the list of widths otherwise."""
    FC, H, shapes = SETS[name]
    out = []
    for g, (B, D, nvec) in enumerate(shapes):
        W, x, _, _ = PC.make_case(B, D, FC, H, nvec, "odd", 1.0, seed=100 + g)
        out.append(({k: v.to(DEV) for k, v in W.items()}, {k: v.to(DEV) for k, v in x.items()},
                    nvec[0] if len(nvec) == 1 else list(nvec)))
    return out


@functools.lru_cache(maxsize=None)
def pair_set(FC, H):
    """The fixtures ``ragged`` and ``full`` of an (FC, H) pair as the two groups, with their references."""
    out = []
    for kind in ("ragged", "full"):
        B, D, nvec, W, x, ref, info = PC.named_case(kind, FC, H)
        out.append(({k: v.to(DEV) for k, v in W.items()}, {k: v.to(DEV) for k, v in x.items()},
                    nvec[0] if len(nvec) == 1 else list(nvec), ref))
    return out


def single(W, x, heads, mode, g):
    """Group g alone through its single operator, out of place: a dict of OUT."""
    key = key_of(g) if mode == P.SAMPLE else None
    h_out = torch.empty_like(x["h"])
    if isinstance(heads, int):
        r = P.policy_step(W, x["obs"], x["done"], x["h"], mode, key=key, h_out=h_out, logits=True)
    else:
        r = P.policy_step_multi(W, x["obs"], x["done"], x["h"], mode, heads, key=key, h_out=h_out, logits=True)
    return dict(zip(OUT, r))


def grouped(groups, mode, order=None, in_place=False):
    """The groups through one launch, in ``order`` (default as listed); results in the listed order."""
    order = list(range(len(groups))) if order is None else list(order)
    hs = [groups[g][1]["h"].clone() if in_place else groups[g][1]["h"] for g in order]
    res = P.policy_step_grouped([groups[g][0] for g in order], [groups[g][1]["obs"] for g in order],
                                [groups[g][1]["done"] for g in order], hs, mode,
                                keys=[key_of(g) for g in order] if mode == P.SAMPLE else None,
                                heads=[groups[g][2] for g in order],
                                h_outs=None if in_place else [torch.empty_like(h) for h in hs], logits=True)
    if in_place:
        assert all(r[0] is h for r, h in zip(res, hs))
    out = [None] * len(groups)
    for g, r in zip(order, res):
        out[g] = dict(zip(OUT, r))
    return out


def assert_equal(got, want, what):
    for k in OUT:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert torch.equal(got[k], want[k]), (what, k)


# ------------------------------------------------------------------ 1. grouped against single launches
@pytest.mark.parametrize("mode", [P.SAMPLE, P.GREEDY])
@pytest.mark.parametrize("name", list(SETS))
def test_grouped_equals_single_bit_for_bit(name, mode):
    groups = group_set(name)
    got = grouped(groups, mode)
    for g, (W, x, heads) in enumerate(groups):
        assert_equal(got[g], single(W, x, heads, mode, g), (name, g))
        assert got[g]["action"].shape == ((x["obs"].shape[0],) if isinstance(heads, int)
                                          else (x["obs"].shape[0], len(heads)))


@pytest.mark.parametrize("FC, H", PC.PAIRS)
def test_every_instantiation_against_single_and_float64(FC, H):
    assert (FC, H) in PC.kernel_pairs()
    groups = pair_set(FC, H)
    for mode in (P.SAMPLE, P.GREEDY):
        got = grouped([g[:3] for g in groups], mode)
        for g, (W, x, heads, ref) in enumerate(groups):
            assert_equal(got[g], single(W, x, heads, mode, g), (FC, H, mode, g))
    for g, (W, x, heads, ref) in enumerate(groups):   # mode 1 (the last launch) against the fixtures' float64
        for k in ("h", "logits", "value", "log_prob"):
            share = PC.bound_share(got[g][k], ref[k])
            assert share <= 1.0, f"FC {FC} H {H} group {g}: {k} uses {share:.3g} of the tolerance"
        want = ref["action"].squeeze(-1) if isinstance(heads, int) else ref["action"]
        assert torch.equal(got[g]["action"].cpu().long(), want), (FC, H, g)


# ------------------------------------------------------------------ 2. robustness of a launch
@pytest.mark.parametrize("mode", [P.SAMPLE, P.GREEDY])
@pytest.mark.parametrize("name", ["ragged", "eight"])
def test_group_order_changes_no_bit(name, mode):
    groups = group_set(name)
    want = grouped(groups, mode)
    got = grouped(groups, mode, order=reversed(range(len(groups))))
    for g in range(len(groups)):
        assert_equal(got[g], want[g], (name, g))


@pytest.mark.parametrize("mode", [P.SAMPLE, P.GREEDY])
def test_one_group_equals_the_plain_operator(mode):
    for g, (W, x, heads) in enumerate(group_set("ragged")):
        got = grouped([(W, x, heads)] * 1, mode, order=[0])
        key = key_of(0) if mode == P.SAMPLE else None
        h_out = torch.empty_like(x["h"])
        if isinstance(heads, int):
            r = P.policy_step(W, x["obs"], x["done"], x["h"], mode, key=key, h_out=h_out, logits=True)
        else:
            r = P.policy_step_multi(W, x["obs"], x["done"], x["h"], mode, heads, key=key, h_out=h_out, logits=True)
        assert_equal(got[0], dict(zip(OUT, r)), g)


@pytest.mark.parametrize("mode", [P.SAMPLE, P.GREEDY])
def test_in_place_carry_equals_out_of_place(mode):
    groups = group_set("ragged")
    want = grouped(groups, mode)
    got = grouped(groups, mode, in_place=True)
    for g in range(len(groups)):
        assert_equal(got[g], want[g], g)


# ------------------------------------------------------------------ 3. rows past B
def test_rows_past_a_groups_B_are_not_written():
    """Every output of every group has 16 guard rows of a sentinel behind it (memory the test owns): they are
    intact after the launch, and every live element has been written."""
    groups = group_set("ragged")
    G, SENT_F, SENT_I = 16, -12345.5, -77
    want = grouped(groups, P.SAMPLE)
    full, views = [], []
    for W, x, heads in groups:
        B, H = x["h"].shape
        K, S = (1, heads) if isinstance(heads, int) else (len(heads), sum(heads))
        t = {"h": torch.full((B + G, H), SENT_F, device=DEV), "log_prob": torch.full((B + G,), SENT_F, device=DEV),
             "value": torch.full((B + G,), SENT_F, device=DEV),
             "action": torch.full((B + G,) if isinstance(heads, int) else (B + G, K), SENT_I, dtype=torch.int32,
                                  device=DEV)}
        full.append(t)
        views.append({k: v[:B] for k, v in t.items()})
    # (the host operator allocates logits itself: the raw entry point takes the guarded ones)
    gs = (_lib.PolicyGroup * len(groups))()
    keep = []
    for g, ((W, x, heads), v, t) in enumerate(zip(groups, views, full)):
        B, D = x["obs"].shape
        hd = [heads] if isinstance(heads, int) else heads
        t["logits"] = torch.full((B + G, sum(hd)), SENT_F, device=DEV)
        v["logits"] = t["logits"][:B]
        r = gs[g]
        r.B, r.D, r.K = B, D, len(hd)
        for k, n in enumerate(hd):
            r.nvec[k] = n
        r.w = P._weights_struct(W, D, W["w_embed"].shape[0], x["h"].shape[1], sum(hd))
        done, key = x["done"].view(torch.uint8), P.head_keys(key_of(g).cpu(), len(hd))
        key = torch.from_numpy(key.view(np.int32).copy()).to(DEV)
        keep += [done, key]
        for name, ten in (("obs", x["obs"]), ("done", done), ("h_in", x["h"]), ("h_out", v["h"]), ("keys", key),
                          ("action", v["action"]), ("log_prob", v["log_prob"]), ("value", v["value"]),
                          ("logits", v["logits"])):
            setattr(r, name, _lib.ptr(ten))
    FC, H, _ = SETS["ragged"]
    _lib.check(_lib.lib().hftlob_policy_step_grouped(FC, H, len(groups), gs, P.SAMPLE, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for g, (v, t) in enumerate(zip(views, full)):
        B = v["h"].shape[0]
        assert_equal(v, want[g], g)
        for k in OUT:
            sent = SENT_I if k == "action" else SENT_F
            assert bool((t[k][B:] == sent).all()), (g, k)


# ------------------------------------------------------------------ 4. graph capture
def test_captured_grouped_launch_replays_bit_for_bit():
    groups = group_set("ragged")
    xs = [{k: v.clone() for k, v in x.items()} for _, x, _ in groups]           # the graph's fixed-address inputs
    keys = [key_of(g).clone() for g in range(len(groups))]
    outs = [(torch.empty(s["action"].shape, dtype=torch.int32, device=DEV), torch.empty_like(s["log_prob"]),
             torch.empty_like(s["value"])) for s in grouped(groups, P.SAMPLE)]
    h_outs = [torch.empty_like(x["h"]) for x in xs]

    def launch():
        return P.policy_step_grouped([W for W, _, _ in groups], [x["obs"] for x in xs], [x["done"] for x in xs],
                                     [x["h"] for x in xs], P.SAMPLE, keys=keys, outs=outs,
                                     heads=[hd for _, _, hd in groups], h_outs=h_outs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for x in xs:                                                                 # new inputs at the same addresses
        x["obs"].mul_(-0.5)
        x["h"].add_(0.25)
        x["done"].logical_not_()
    for g, k in enumerate(keys):
        k.copy_(key_of(g + 40))
    for t in h_outs + [o for out in outs for o in out]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for g, ((W, _, heads), x) in enumerate(zip(groups, xs)):
        want = single(W, x, heads, P.SAMPLE, g + 40)
        got = dict(zip(OUT, (h_outs[g],) + outs[g]))
        for k in ("h", "action", "log_prob", "value"):
            assert torch.equal(got[k], want[k]), (g, k)


# ------------------------------------------------------------------ 5. error codes
def test_abi_error_codes():
    L = _lib.lib()
    fn = L.hftlob_policy_step_grouped
    EINVAL, ENULL, ESHAPE = -1, -2, -3
    k = 64   # never dereferenced: every call below fails a host check, which runs before any device call

    def rows(n, **edit):
        """n groups of valid sizes and non-NULL pointers; ``edit`` changes fields of the LAST group."""
        gs = (_lib.PolicyGroup * max(n, 1))()
        for g in range(max(n, 1)):
            r = gs[g]
            r.B, r.D, r.K = 4, 3, 2
            r.nvec[0], r.nvec[1] = 5, 16
            for name, _ in _lib.PolicyWeights._fields_:
                setattr(r.w, name, k)
            for name in ("obs", "done", "h_in", "h_out", "keys", "action", "log_prob", "value", "logits"):
                setattr(r, name, k)
        last = gs[max(n, 1) - 1]
        for name, v in edit.items():
            if name == "nvec1":
                last.nvec[1] = v
            elif name.startswith("w."):
                setattr(last.w, name[2:], v)
            else:
                setattr(last, name, v)
        return gs

    def call(code, n, gs, FC=64, H=64, mode=0, names=()):
        assert fn(FC, H, n, gs, mode, None) == code, (n, FC, H, mode)
        msg = L.hftlob_last_error()
        assert b"policy_step_grouped" in msg, msg
        for s in names:
            assert s in msg, (s, msg)

    for n in (0, 9, -1):
        call(ESHAPE, n, rows(9), names=[b"n_groups"])
    call(ENULL, 2, C.POINTER(_lib.PolicyGroup)(), names=[b"groups is NULL"])
    for H in (32, 96, 512):
        call(ESHAPE, 2, rows(2), H=H)
        call(ESHAPE, 2, rows(2), FC=H)
    call(ESHAPE, 3, rows(3, B=0), names=[b"group 2", b"B must"])
    call(ESHAPE, 2, rows(2, D=65), names=[b"group 1"])
    call(ESHAPE, 2, rows(2, K=5), names=[b"group 1"])
    call(ESHAPE, 3, rows(3, nvec1=17), names=[b"group 2", b"nvec"])
    call(ESHAPE, 1, rows(1, nvec1=0), names=[b"group 0"])
    call(EINVAL, 2, rows(2), mode=2, names=[b"mode"])
    for name in ("obs", "done", "h_in", "h_out", "keys", "action", "log_prob", "value", "w.w_embed", "w.b_a2"):
        call(ENULL, 3, rows(3, **{name: None}), names=[b"group 2"])
    call(EINVAL, 2, rows(2, **{"w.w_ih": k + 4}), names=[b"group 1", b"16-byte aligned"])
    # the first group at fault is the one reported
    gs = rows(3, B=0)
    gs[1].B = -1
    call(ESHAPE, 3, gs, names=[b"group 1"])
