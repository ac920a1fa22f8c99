"""The grouped GRU scan on the GPU (hftlob_gru_scan_fwd_grouped / _bwd_grouped, hftlob.train.gru's grouped
operators and GRUScanGrouped, the learner's GROUPED_SCAN switch).  Every group of a grouped launch must
equal bit for bit what the single-batch operators give for that group alone; each case is also held to
the float64 CPU restatement under the bound of tests/test_gpu_gru_scan.py: per tensor
|got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, and exactly 0 where the whole reference tensor is 0.

The shapes are the smallest at which the tile and group arithmetic can go wrong: a group of one row, of
exactly one tile and of a tile plus one row; a group behind one that ends inside a tile; the full K loop
of H = 256; eight groups; one group."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.train import gru as G
from hftlob.train import ippo as I

pytestmark = pytest.mark.gpu

# (T, H, the groups' B, the groups that are all-done at t = 0 and t = 2)
CASES = {"1_16_17": (3, 64, (1, 16, 17), ()), "33_5": (8, 256, (33, 5), ()), "17_17_40": (5, 128, (17, 17, 40), (2,)),
         "eight": (1, 64, (1, 2, 3, 4, 5, 6, 7, 8), ()), "one": (4, 64, (19,), ())}
FWD = ("gi", "h0", "done", "w_hh", "b_hh")


def assert_close(name, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert not got.any(), f"{name}: reference is 0 everywhere, got max |x| = {float(got.abs().max())}"
        return
    worst = float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * scale)).max())
    print(f"{name}: max error / bound = {worst:.4f}")
    assert worst <= 1.0, f"{name}: max error / bound = {worst}"


def make_group(T, B, H, all0, seed):
    """One group's float32 inputs, generated as case() of tests/test_gpu_gru_scan.py generates them (non-zero
    b_hh, d_hseq non-zero at every t, done at rate 0.3), and the float64 CPU reference of every output."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    done = torch.rand(T, B, generator=g) < 0.3
    done[0] = torch.arange(B) % 2 == 1
    if all0:
        done[0] = True
        done[2] = True
    x = dict(gi=r(T, B, 3 * H), h0=r(B, H), done=done, w_hh=r(3 * H, H) / H ** 0.5, b_hh=0.5 * r(3 * H),
             d_hseq=r(T, B, H))
    d = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in x.items()}
    hseq, gates = G.gru_scan_reference(d["gi"], d["h0"], d["done"], d["w_hh"], d["b_hh"])
    d_gi, d_gh_n, d_h0 = G.gru_scan_backward_reference(d["d_hseq"], hseq, gates, d["h0"], d["done"], d["w_hh"])
    return x, dict(hseq=hseq, gates=gates, d_gi=d_gi, d_gh_n=d_gh_n, d_h0=d_h0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs on the device, float64 references, single-batch operator outputs) per group; computed once
    per case and not modified by the tests."""
    T, H, Bs, all0 = CASES[name]
    xs, refs, single = [], [], []
    for k, B in enumerate(Bs):
        x, ref = make_group(T, B, H, k in all0, seed=1000 * k + 7 * T + 31 * B + H)
        c = {key: v.cuda() for key, v in x.items()}
        hseq, gates = G.scan_forward(*(c[key] for key in FWD), save_gates=True)
        d_gi, d_gh_n, d_h0 = G.scan_backward(c["d_hseq"], hseq, gates, c["h0"], c["done"], c["w_hh"])
        xs.append(c), refs.append(ref)
        single.append(dict(hseq=hseq, gates=gates, d_gi=d_gi, d_gh_n=d_gh_n, d_h0=d_h0))
    torch.cuda.synchronize()
    return xs, refs, single


def grouped(xs, single, order=None, save=True):
    """The grouped forward on the inputs and the grouped backward on the single-batch forward's outputs
    (the same inputs the single-batch backward had), in ``order``; per group, in the original order."""
    order = list(range(len(xs))) if order is None else list(order)
    fw = G.scan_forward_grouped([tuple(xs[k][key] for key in FWD) for k in order], save_gates=save)
    bw = G.scan_backward_grouped([(xs[k]["d_hseq"], single[k]["hseq"], single[k]["gates"], xs[k]["h0"], xs[k]["done"],
                                   xs[k]["w_hh"]) for k in order])
    out = [None] * len(xs)
    for pos, k in enumerate(order):
        out[k] = dict(hseq=fw[pos][0], gates=fw[pos][1], d_gi=bw[pos][0], d_gh_n=bw[pos][1], d_h0=bw[pos][2])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_grouped_equals_single_bit_for_bit(name):
    xs, refs, single = case(name)
    got = grouped(xs, single)
    for k, (g, s, ref) in enumerate(zip(got, single, refs)):
        for key in ("hseq", "gates", "d_gi", "d_gh_n", "d_h0"):
            assert torch.equal(g[key], s[key]), f"group {k}: {key} differs from the single-batch operator"
            assert_close(f"group {k} {key}", g[key], ref[key])
    if CASES[name][3]:
        for k in CASES[name][3]:
            assert not refs[k]["d_h0"].any() and not got[k]["d_h0"].any()


@pytest.mark.parametrize("name", ["1_16_17", "17_17_40"])
def test_group_order_changes_no_bit(name):
    xs, _, single = case(name)
    got = grouped(xs, single, order=reversed(range(len(xs))))
    for k, (g, s) in enumerate(zip(got, single)):
        for key in ("hseq", "gates", "d_gi", "d_gh_n", "d_h0"):
            assert torch.equal(g[key], s[key]), (k, key)


def test_gates_null_for_some_groups_changes_no_hseq():
    xs, _, single = case("1_16_17")
    for save in ([True, False, True], [False, True, False], [False, False, False]):
        fw = G.scan_forward_grouped([tuple(x[key] for key in FWD) for x in xs], save_gates=save)
        for k, ((hseq, gates), s) in enumerate(zip(fw, single)):
            assert (gates is not None) == save[k]
            assert torch.equal(hseq, s["hseq"]), (save, k)
            if gates is not None:
                assert torch.equal(gates, s["gates"]), (save, k)


def _fwd_rows(rows):
    return (_lib.GruFwdGroup * len(rows))(*[_lib.GruFwdGroup(*r) for r in rows])


def _bwd_rows(rows):
    return (_lib.GruBwdGroup * len(rows))(*[_lib.GruBwdGroup(*r) for r in rows])


def test_rows_past_a_groups_B_are_not_written():
    """B = (17, 1): group 0's second tile has one live row, group 1's only tile one.  Every output of every
    group is allocated with one spare tile of rows behind it, filled with a sentinel that must be intact
    afterwards (memory the test owns), and every live element must have been written."""
    T, H, TILE, S = 5, 128, 16, -12345.0
    Bs = (17, 1)
    L, p = _lib.lib(), _lib.ptr
    made = [make_group(T, B, H, False, seed=50 + B) for B in Bs]
    xs = [{k: v.cuda() for k, v in x.items()} for x, _ in made]

    def padded(rows, width):
        return torch.full((rows + TILE, width), S, dtype=torch.float32, device="cuda")

    bufs = [dict(hseq=padded(T * B, H), gates=padded(T * B, 4 * H), d_gi=padded(T * B, 3 * H), d_gh_n=padded(T * B, H),
                 d_h0=padded(B, H)) for B in Bs]
    dones = [x["done"].view(torch.uint8) for x in xs]
    fw = _fwd_rows([(B, p(x["gi"]), p(x["h0"]), p(d), p(x["w_hh"]), p(x["b_hh"]), p(b["hseq"]), p(b["gates"]))
                    for B, x, d, b in zip(Bs, xs, dones, bufs)])
    _lib.check(L.hftlob_gru_scan_fwd_grouped(T, H, 2, fw, _lib.stream_ptr()))
    bw = _bwd_rows([(B, p(x["d_hseq"]), p(b["hseq"]), p(b["gates"]), p(x["h0"]), p(d), p(x["w_hh"]), p(b["d_gi"]),
                     p(b["d_gh_n"]), p(b["d_h0"])) for B, x, d, b in zip(Bs, xs, dones, bufs)])
    _lib.check(L.hftlob_gru_scan_bwd_grouped(T, H, 2, bw, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, (B, b, (_, ref)) in enumerate(zip(Bs, bufs, made)):
        for name, buf in b.items():
            rows = B if name == "d_h0" else T * B
            assert bool((buf[rows:] == S).all()), f"group {k} {name}: rows past B were written"
            assert not bool((buf[:rows] == S).any()), f"group {k} {name}: a live element was not written"
            assert_close(f"group {k} {name}", buf[:rows].view(ref[name].shape), ref[name])


def _leaves(x):
    return {k: x[k].clone().requires_grad_(True) for k in ("gi", "h0", "w_hh", "b_hh")}


def test_autograd_function_equals_gru_scan_per_group():
    xs, _, _ = case("17_17_40")
    want = []
    for x in xs:
        lv = _leaves(x)
        hseq = G.gru_scan(lv["gi"], lv["h0"], x["done"], lv["w_hh"], lv["b_hh"])
        hseq.backward(x["d_hseq"])
        want.append((hseq.detach(), {k: v.grad for k, v in lv.items()}))
    lvs = [_leaves(x) for x in xs]
    hseqs = G.gru_scan_grouped(*([lv[k] for lv in lvs] for k in ("gi", "h0")), [x["done"] for x in xs],
                               *([lv[k] for lv in lvs] for k in ("w_hh", "b_hh")))
    assert isinstance(hseqs, tuple) and len(hseqs) == 3
    torch.autograd.backward(list(hseqs[:2]), [x["d_hseq"] for x in xs[:2]])   # group 2's hseq gets no gradient
    for k, (lv, (hseq, grads)) in enumerate(zip(lvs, want)):
        assert torch.equal(hseqs[k], hseq), k
        for key in ("gi", "h0", "w_hh", "b_hh"):
            if k < 2:
                assert torch.equal(lv[key].grad, grads[key]), (k, key)
            else:   # autograd's materialised zeros went through the backward: every gradient is 0
                assert lv[key].grad is not None and not lv[key].grad.any(), (k, key)
    with torch.no_grad():   # no input needs a gradient: gates = NULL for every group
        plain = G.gru_scan_grouped(*([x[k] for x in xs] for k in FWD))
    assert all(torch.equal(a, b[0]) for a, b in zip(plain, want))


def test_groups_sharing_one_w_hh_leaf_accumulate_into_it():
    xs, _, _ = case("17_17_40")
    a, b = xs[0], xs[1]
    w, bias = a["w_hh"].clone().requires_grad_(True), a["b_hh"].clone().requires_grad_(True)
    each = []
    for x in (a, b):
        wl, bl = a["w_hh"].clone().requires_grad_(True), a["b_hh"].clone().requires_grad_(True)
        G.gru_scan(x["gi"], x["h0"], x["done"], wl, bl).backward(x["d_hseq"])
        each.append((wl.grad, bl.grad))
    hs = G.gru_scan_grouped([a["gi"], b["gi"]], [a["h0"], b["h0"]], [a["done"], b["done"]], [w, w], [bias, bias])
    torch.autograd.backward(list(hs), [a["d_hseq"], b["d_hseq"]])
    assert torch.equal(w.grad, each[0][0] + each[1][0]) and torch.equal(bias.grad, each[0][1] + each[1][1])


def test_captured_grouped_scan_replays_bit_for_bit():
    """A grouped forward and backward inside one torch.cuda.graph (warm-up on a side stream); a replay after
    the inputs are overwritten equals the eager call on the new inputs."""
    T, H, Bs = 3, 64, (17, 5)
    static = [{k: v.cuda() for k, v in make_group(T, B, H, False, seed=70 + B)[0].items()} for B in Bs]

    def run(xs):
        fw = G.scan_forward_grouped([tuple(x[key] for key in FWD) for x in xs])
        bw = G.scan_backward_grouped([(x["d_hseq"], h, g, x["h0"], x["done"], x["w_hh"]) for x, (h, g) in zip(xs, fw)])
        return [t for pair in fw for t in pair] + [t for tri in bw for t in tri]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    new = [{k: v.cuda() for k, v in make_group(T, B, H, False, seed=90 + B)[0].items()} for B in Bs]
    for s, n in zip(static, new):
        for k, v in n.items():
            s[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(new)
    assert len(outs) == len(eager) == 10
    for i, (a, b) in enumerate(zip(outs, eager)):
        assert torch.equal(a, b), i
    assert not torch.equal(eager[0], run([{k: v.cuda() for k, v in make_group(T, B, H, False, seed=70 + B)[0].items()}
                                          for B in Bs])[0])   # (and the new inputs are other inputs)


def test_abi_error_codes():
    L = _lib.lib()
    ENULL, ESHAPE = -2, -3
    k = 64   # never dereferenced: the checks run on the host before any device call
    fwd, bwd = L.hftlob_gru_scan_fwd_grouped, L.hftlob_gru_scan_bwd_grouped
    gf, gb = (4,) + (k,) * 6 + (None,), (4,) + (k,) * 9        # forward: gates may be NULL
    null_f = C.POINTER(_lib.GruFwdGroup)()
    null_b = C.POINTER(_lib.GruBwdGroup)()

    def both(code, T, H, n, rows_f, rows_b):
        assert fwd(T, H, n, rows_f, None) == code, (T, H, n)
        assert b"gru_scan" in L.hftlob_last_error()
        assert bwd(T, H, n, rows_b, None) == code, (T, H, n)
        assert b"gru_scan" in L.hftlob_last_error()

    two_f, two_b = _fwd_rows([gf, gf]), _bwd_rows([gb, gb])
    for n in (0, -1, 9):
        both(ESHAPE, 4, 64, n, _fwd_rows([gf] * 9), _bwd_rows([gb] * 9))
    for T in (0, -1):
        both(ESHAPE, T, 64, 2, two_f, two_b)
    for H in (32, 96, 0, 512):
        both(ESHAPE, 4, H, 2, two_f, two_b)
    for B in (0, -3):
        both(ESHAPE, 4, 64, 2, _fwd_rows([gf, (B,) + gf[1:]]), _bwd_rows([gb, (B,) + gb[1:]]))
    both(ENULL, 4, 64, 2, null_f, null_b)
    for i in range(1, 7):                                       # every forward array but gates
        r = list(gf)
        r[i] = None
        assert fwd(4, 64, 2, _fwd_rows([gf, tuple(r)]), None) == ENULL, i
        assert b"gru_scan" in L.hftlob_last_error()
    for i in range(1, 10):
        r = list(gb)
        r[i] = None
        assert bwd(4, 64, 2, _bwd_rows([gb, tuple(r)]), None) == ENULL, i
        assert b"gru_scan" in L.hftlob_last_error()


# ------------------------------------------------------------------ the trainer
@functools.lru_cache(maxsize=None)
def make_env(name):
    cfg = builtin_config(name)
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=False, persistent_outputs=True), cfg


def config(cfg, **kw):
    return I.default_config(NUM_ENVS=16, NUM_STEPS=8, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, UPDATE_EPOCHS=2,
                            NUM_MINIBATCHES=2, TOTAL_TIMESTEPS=16 * 8 * 8, FUSED_GRU=True, FUSED_POLICY=True,
                            FUSED_LOSS=True, FUSED_OPT=True, NUM_AGENTS_PER_TYPE=cfg.number_of_agents_per_type, **kw)


def run_pair(name, graphs, updates, monkeypatch):
    """A trainer without and one with the switch, ``updates`` updates each.  Counts the Python calls of the two
    scans: every minibatch step of the plain trainer is one ``gru_scan`` of its type's net, every one of the joint
    trainer one ``gru_scan_grouped`` of all the nets, and neither trainer calls the other's."""
    env, cfg = make_env(name)
    calls = {"gru_scan": 0, "gru_scan_grouped": 0}

    def counted(fn, real):
        def wrapper(*a, **k):
            calls[fn] += 1
            return real(*a, **k)
        return wrapper

    for fn in calls:
        monkeypatch.setattr(I, fn, counted(fn, getattr(I, fn)))
    # a step group's Python runs per update: each of its 2 x 2 steps when eager; under graphs the two warm-ups and
    # the capture, all in the first update, and then replays, which call no Python: the counts stop growing
    runs_per_update = ([3] + [0] * (updates - 1)) if graphs else [4] * updates
    runs = []
    for grouped_scan in (False, True):
        tr = I.IPPOTrainer(env, config(cfg, CUDA_GRAPHS=graphs, GROUPED_SCAN=grouped_scan))
        assert tr.grouped_scan is grouped_scan and tr.graphs is graphs
        losses, counts = [], []
        for _ in range(updates):
            before = dict(calls)
            m = tr.update()
            counts.append(tuple(calls[fn] - before[fn] for fn in ("gru_scan", "gru_scan_grouped")))
            losses.append([{k: v.clone() for k, v in d.items()} for d in m["loss"]])
        if grouped_scan:
            assert counts == [(0, k) for k in runs_per_update], counts
        else:
            assert counts == [(tr.n_types * k, 0) for k in runs_per_update], counts
        runs.append((tr, losses))
    torch.cuda.synchronize()
    return runs


def assert_same_training(plain, joint, updates):
    (a, la), (b, lb) = plain, joint
    assert a.opt_count == b.opt_count == [4 * updates] * a.n_types
    assert torch.equal(a.gen.get_state(), b.gen.get_state())
    for i in range(a.n_types):
        for (name, p), q in zip(a.nets[i].named_parameters(), b.nets[i].parameters()):
            assert torch.equal(p, q), f"type {i}: {name}"
            sa, sb = a.opts[i].state[p], b.opts[i].state[q]
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sa[key], sb[key]), f"type {i}: {name} {key}"
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(a.buf[i], f.name), getattr(b.buf[i], f.name)), (i, f.name)
    for u, (da, db) in enumerate(zip(la, lb)):
        for i, (x, y) in enumerate(zip(da, db)):
            for key in x:
                assert np.isfinite(float(x[key])) and torch.equal(x[key], y[key]), (u, i, key)


@pytest.mark.parametrize("graphs", [False, True])
def test_trainer_with_and_without_the_switch_two_types(graphs, monkeypatch):
    """Four updates of 2 x 2 minibatch steps; with graphs the joint step is warmed up, captured and replayed."""
    plain, joint = run_pair("2_player_fq_fqc", graphs, 4, monkeypatch)
    assert_same_training(plain, joint, 4)
    tr = joint[0]
    assert all(n.fused for n in tr.nets)
    if graphs:
        assert [s["types"] for s in tr._steps] == [list(range(tr.n_types))]   # (one joint step and no per-type one)
        assert isinstance(tr._steps[0]["graph"], torch.cuda.CUDAGraph)
        assert [s["types"] for s in plain[0]._steps] == [[i] for i in range(plain[0].n_types)]
        assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in plain[0]._steps)
    else:
        assert [s["graph"] for s in tr._steps] == [None]


def test_trainer_with_and_without_the_switch_three_types(monkeypatch):
    plain, joint = run_pair("3_player_fq_fqc_dir", False, 2, monkeypatch)
    assert joint[0].n_types == 3
    assert_same_training(plain, joint, 2)


def test_restored_trainer_goes_on_with_the_switch(tmp_path):
    env, cfg = make_env("2_player_fq_fqc")
    src = I.IPPOTrainer(env, config(cfg, CUDA_GRAPHS=True, GROUPED_SCAN=True))
    src.update()
    assert [s["types"] for s in src._steps] == [list(range(src.n_types))]
    assert isinstance(src._steps[0]["graph"], torch.cuda.CUDAGraph)
    path = str(tmp_path / "ck.pt")
    src.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["format"] == I.CHECKPOINT_FORMAT and ck["config"]["GROUPED_SCAN"] is True
    dst = I.IPPOTrainer(env, config(cfg, CUDA_GRAPHS=True, GROUPED_SCAN=True, SEED=3))
    dst.update()
    dst.load_checkpoint(path)
    assert [s["types"] for s in dst._steps] == [list(range(dst.n_types))]
    assert dst._steps[0]["graph"] is None and dst._steps[0]["warm"] == 0   # dropped: captured again at the next update
    for i in range(src.n_types):
        for p, q in zip(src.nets[i].parameters(), dst.nets[i].parameters()):
            assert torch.equal(p, q)
    m = dst.update()
    assert all(np.isfinite(float(v)) for d in m["loss"] for v in d.values())
    assert isinstance(dst._steps[0]["graph"], torch.cuda.CUDAGraph) and dst.opt_count == [8, 8]
    for i in range(dst.n_types):
        assert all(float(dst.opts[i].state[p]["step"]) == 8.0 for p in dst.nets[i].parameters())
