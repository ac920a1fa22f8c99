"""The update's fused global-norm clip and Adam step on the GPU (hftlob_adam_clip, hftlob.train.optim, the
learner's FUSED_OPT switch), held to the float64 CPU restatement (adam_clip_reference) evaluated from the
same float32 inputs.  The bound is the project's form (tests/test_gpu_ppo_loss.py): per element
|got - ref| <= 1e-5 (|ref| + scale), where scale is lr, the size of one Adam step, for a parameter and
the tensor's mean |ref| for exp_avg and exp_avg_sq; total_norm within 1e-5 ref.  Where the reference and
its scale are 0 the result must be 0 exactly.  Every comparison prints its error over the bound, and so
does torch's own float32 path on the CPU (clip_grad_norm_ + Adam.step()) on the same inputs: what any
float32 code uses of the bound.

The gradients are scaled to a chosen global norm, so the clip is well inside (norm 4 max_norm) or well
outside (norm max_norm / 5) its range: a float32 evaluation may not take the other side than float64."""
import copy
import dataclasses
import functools

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.train import ippo as I
from hftlob.train import optim as OP

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, MAX_NORM = 2.5e-4, 0.9, 0.999, 1e-5, 0.5
CH = OP.CHUNK
# one element; a short quad; one short of, exactly and one past a chunk; tensors of several chunks next
# to tiny ones; 16 tensors with every kind of tail; more chunks than the norm pass has workgroups
SIZES = {"1": [1], "3": [3], "chunk-1": [CH - 1], "chunk": [CH], "chunk+1": [CH + 1],
         "mixed4": [4 * CH + 1, 1, 7, 2 * CH],
         "mixed16": [1, 3, CH, 5, CH + 3, 1, 17, 2 * CH - 1, 64, 1, 255, 256, 257, 4, 1023, 2],
         "65chunks": [65 * CH + 5]}
assert len(SIZES["mixed16"]) == OP.MAX_TENSORS and 65 > OP.WORKSPACE


@functools.lru_cache(maxsize=None)
def case(name, grad_norm, step0, lr=LR, zero_p=False):
    """Float32 inputs on the CPU and the float64 reference of every output; computed once per case and not
    modified by the tests.  ``step0``: one entering step for every tensor, or a tuple with each tensor's
    own.  A tensor entering at step 0 has zero state, the others a plausible one (|exp_avg| of the order
    of sqrt(exp_avg_sq), so a step of the order of lr)."""
    sizes = SIZES[name]
    steps = list(step0) if isinstance(step0, tuple) else [step0] * len(sizes)
    g = torch.Generator().manual_seed(sum(sizes) + 31 * len(sizes) + int(1000 * grad_norm) + int(sum(steps)))
    r = lambda n: torch.randn(n, generator=g, dtype=torch.float32)  # noqa: E731
    p = [torch.zeros(n) if zero_p else r(n) for n in sizes]
    grads = [r(n) for n in sizes]
    norm = float(torch.sqrt(sum((x.double() ** 2).sum() for x in grads)))
    grads = [x * (grad_norm / norm) if grad_norm > 0 else torch.zeros_like(x) for x in grads]
    m = [0.01 * r(n) if s else torch.zeros(n) for n, s in zip(sizes, steps)]
    v = [1e-4 * (0.25 + r(n) ** 2) if s else torch.zeros(n) for n, s in zip(sizes, steps)]
    x = dict(p=p, g=grads, m=m, v=v, steps=[float(s) for s in steps], lr=lr)
    d = lambda ts: [t.double() for t in ts]  # noqa: E731
    ref = OP.adam_clip_reference(d(p), d(grads), d(m), d(v), x["steps"], float(np.float32(lr)), B1, B2, EPS, MAX_NORM)
    if grad_norm > 0:   # the case is on the side of the clip it was made for
        assert (float(ref[4]) >= 2 * MAX_NORM) if grad_norm > MAX_NORM else (float(ref[4]) <= 0.5 * MAX_NORM)
    return x, dict(p=ref[0], m=ref[1], v=ref[2], steps=[float(s) for s in ref[3]], total=float(ref[4]))


def run_op(x, total_norm=True):
    """hftlob_adam_clip through the C ABI on device copies of the case: dict of the device tensors after
    the call (p, g, m, v, steps, total)."""
    dev = {k: [t.cuda() for t in x[k]] for k in ("p", "g", "m", "v")}
    dev["steps"] = [torch.tensor(s, dtype=torch.float32, device="cuda") for s in x["steps"]]
    lr = torch.tensor(x["lr"], dtype=torch.float32, device="cuda")
    ws = torch.empty(OP.WORKSPACE, dtype=torch.float64, device="cuda")
    dev["total"] = torch.full((), -1.0, dtype=torch.float32, device="cuda") if total_norm else None
    n = len(x["p"])
    arr = (_lib.AdamTensor * n)(*[_lib.AdamTensor(*[_lib.ptr(dev[k][i]) for k in ("p", "g", "m", "v", "steps")],
                                                  dev["p"][i].numel()) for i in range(n)])
    _lib.check(_lib.lib().hftlob_adam_clip(n, arr, _lib.ptr(lr), B1, B2, EPS, MAX_NORM, _lib.ptr(ws),
                                           _lib.ptr(dev["total"]), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dev


def over_bound(name, got, ref, scale):
    """max |got - ref| / (1e-5 (|ref| + scale)); where the bound is 0 the error must be."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, bound = (got - ref).abs(), 1e-5 * (ref.abs() + scale)
    if not bool((err[bound == 0] == 0).all()):
        return float("inf")                             # the bound is 0 there, the error is not
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def assert_outputs(label, got, ref, lr, enforce=True):
    """p, m, v of every tensor and total_norm within the bound; prints and returns the largest error over
    it.  ``enforce`` off: the figures are printed only (torch's own path is not what is under test)."""
    worst = {}
    for k in ("p", "m", "v"):
        ws = [over_bound(f"{label} {k}[{i}]", a, b, lr if k == "p" else float(b.abs().mean()))
              for i, (a, b) in enumerate(zip(got[k], ref[k]))]
        worst[k] = max(ws)
    if got.get("total") is not None:
        t, rt = float(got["total"]), ref["total"]
        worst["total_norm"] = abs(t - rt) / (1e-5 * rt) if rt > 0 else (0.0 if t == 0.0 else float("inf"))
    print(f"{label}: error / bound " + ", ".join(f"{k} {w:.4f}" for k, w in worst.items()))
    for k, w in worst.items():
        assert w <= 1.0 or not enforce, f"{label} {k}: error / bound = {w}"
    return max(worst.values())


def torch_cpu_path(x):
    """clip_grad_norm_ + torch.optim.Adam.step() in float32 on the CPU from the case's inputs and state."""
    ps = [torch.nn.Parameter(t.clone()) for t in x["p"]]
    opt = torch.optim.Adam(ps, lr=x["lr"], betas=(B1, B2), eps=EPS)
    for p, g, m, v, s in zip(ps, x["g"], x["m"], x["v"], x["steps"]):
        p.grad = g.clone()
        opt.state[p] = {"step": torch.tensor(s), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    total = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
    opt.step()
    return dict(p=[p.detach() for p in ps], m=[opt.state[p]["exp_avg"] for p in ps],
                v=[opt.state[p]["exp_avg_sq"] for p in ps], total=total)


def check_case(x, ref, label):
    snap = copy.deepcopy(x)
    got = run_op(x)
    assert_outputs(f"fused {label}", got, ref, x["lr"])
    assert [float(s) for s in got["steps"]] == ref["steps"] == [s + 1.0 for s in x["steps"]]
    for a, b in zip(got["g"], x["g"]):
        assert torch.equal(a.cpu(), b)                   # the gradients are read only
    assert_outputs(f"float32 CPU torch {label}", torch_cpu_path(x), ref, x["lr"], enforce=False)
    for k in ("p", "g", "m", "v"):
        assert all(torch.equal(a, b) for a, b in zip(x[k], snap[k]))   # (the shared case is as it was)
    return got


# ------------------------------------------------------------------ the operator against float64
@pytest.mark.parametrize("step0", [0, 1000])
@pytest.mark.parametrize("grad_norm", [4 * MAX_NORM, MAX_NORM / 5], ids=["clip_active", "clip_inactive"])
@pytest.mark.parametrize("name", list(SIZES))
def test_step_matches_float64(name, grad_norm, step0):
    x, ref = case(name, grad_norm, step0)
    got = check_case(x, ref, f"{name} norm {grad_norm} step {step0}")
    if grad_norm > MAX_NORM:     # the clip took part: exp_avg from step 0 is that of the scaled gradient
        coef = MAX_NORM / (ref["total"] + 1e-6)
        assert 0.2 < coef < 0.3
        if step0 == 0:
            assert torch.allclose(got["m"][0].cpu().double(), x["g"][0].double() * coef * (1 - B1), rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", ["3", "mixed4", "mixed16"])
def test_zero_gradient(name):
    """coef = 1 (0 / 1e-6 clamps), p unchanged apart from the decaying exp_avg's step, m and v decayed."""
    x, ref = case(name, 0.0, 1000)
    got = check_case(x, ref, f"{name} zero gradient")
    assert float(got["total"]) == 0.0
    for a, m, v, m0, v0 in zip(got["g"], got["m"], got["v"], x["m"], x["v"]):
        assert not a.any()
        assert torch.equal(m.cpu(), m0 + (0.0 - m0) * torch.tensor(1.0 - B1, dtype=torch.float32))
        assert torch.equal(v.cpu(), v0 * torch.tensor(B2, dtype=torch.float32))
    x, ref = case(name, 0.0, 0)      # from zero state: nothing moves at all
    got = check_case(x, ref, f"{name} zero gradient, zero state")
    for k in ("p", "m", "v"):
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got[k], x[k])), k


@pytest.mark.parametrize("name", ["chunk+1", "mixed16"])
def test_lr_zero_leaves_the_parameters_bit_identical(name):
    x, ref = case(name, 4 * MAX_NORM, 1000, lr=0.0)
    got = check_case(x, ref, f"{name} lr 0")
    for a, b, m, m0, v, v0 in zip(got["p"], x["p"], got["m"], x["m"], got["v"], x["v"]):
        assert torch.equal(a.cpu(), b)
        assert not torch.equal(m.cpu(), m0) and not torch.equal(v.cpu(), v0)


@pytest.mark.parametrize("step0", [0, 1000])
@pytest.mark.parametrize("name", ["mixed4", "mixed16"])
def test_zero_parameters_bound_the_step_itself(name, step0):
    """Every p = 0: the bound on p is 1e-5 (|step| + lr), not hidden behind 1e-5 |p|."""
    x, ref = case(name, MAX_NORM / 5, step0, zero_p=True)
    assert all(not t.any() for t in x["p"]) and all(float(t.abs().max()) <= 20 * LR for t in ref["p"])
    got = check_case(x, ref, f"{name} p = 0 step {step0}")
    assert all(bool(t.any()) for t in got["p"])


@pytest.mark.parametrize("name,steps", [("mixed4", (0, 1000, 1, 7)),
                                        ("mixed16", tuple([0, 1, 2, 1000, 5, 0, 33, 1, 0, 250, 3, 0, 1, 999, 12, 4]))])
def test_every_tensor_uses_its_own_step(name, steps):
    x, ref = case(name, MAX_NORM / 5, steps)
    got = check_case(x, ref, f"{name} own steps")
    assert [float(s) for s in got["steps"]] == [s + 1.0 for s in steps]
    # and not another's: with every step set to the first tensor's, the later tensors' parameters differ
    same = dict(x, steps=[float(steps[0])] * len(steps))
    other = run_op(same)
    assert torch.equal(other["p"][0], got["p"][0]) and not torch.equal(other["p"][1], got["p"][1])


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("name", ["3", "mixed16", "65chunks"])
def test_two_calls_give_the_same_bits_and_total_norm_may_be_null(name):
    x, _ = case(name, 4 * MAX_NORM, 1000)
    a, b, c = run_op(x), run_op(x), run_op(x, total_norm=False)
    assert c["total"] is None and torch.equal(a["total"], b["total"])
    for k in ("p", "m", "v", "steps", "g"):
        for s, t, u in zip(a[k], b[k], c[k]):
            assert torch.equal(s, t) and torch.equal(s, u), k


def test_stores_stay_inside_their_tensors():
    """Tensors of 1025, 3 and 1 elements carved out of one buffer each, 16-byte aligned, with sentinel
    floats between and behind them that must be intact afterwards (memory the test owns)."""
    sizes, PAD, S = [CH + 1, 3, 1], 64, -12345.0
    g = torch.Generator().manual_seed(3)
    vals = {k: [torch.randn(n, generator=g).abs() * 1e-3 for n in sizes] for k in ("p", "g", "m", "v")}
    want = run_op(dict(vals, steps=[0.0, 5.0, 9.0], lr=LR))
    offs = np.cumsum([0] + [((n + 3) // 4) * 4 + PAD for n in sizes])
    bufs = {k: torch.full((int(offs[-1]),), S, dtype=torch.float32, device="cuda") for k in ("p", "g", "m", "v")}
    steps = torch.full((3 + PAD,), S, dtype=torch.float32, device="cuda")
    steps[:3] = torch.tensor([0.0, 5.0, 9.0])
    ws = torch.full((OP.WORKSPACE + PAD,), S, dtype=torch.float64, device="cuda")
    total = torch.full((1 + PAD,), S, dtype=torch.float32, device="cuda")
    lr = torch.tensor(LR, dtype=torch.float32, device="cuda")
    views = {k: [bufs[k][int(o):int(o) + n] for o, n in zip(offs, sizes)] for k in bufs}
    for k in bufs:
        for t, s in zip(views[k], vals[k]):
            t.copy_(s)
    arr = (_lib.AdamTensor * 3)(*[_lib.AdamTensor(*[views[k][i].data_ptr() for k in ("p", "g", "m", "v")],
                                                  steps[i:].data_ptr(), sizes[i]) for i in range(3)])
    _lib.check(_lib.lib().hftlob_adam_clip(3, arr, _lib.ptr(lr), B1, B2, EPS, MAX_NORM, _lib.ptr(ws), _lib.ptr(total),
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "g"):
        live = torch.zeros(int(offs[-1]), dtype=torch.bool, device="cuda")
        for i, (o, n) in enumerate(zip(offs, sizes)):
            assert torch.equal(views[k][i], want[k][i]), (k, i)
            live[int(o):int(o) + n] = True
        assert bool((bufs[k][~live] == S).all()), f"{k}: written outside its tensors"
    assert steps[:3].tolist() == [1.0, 6.0, 10.0] and bool((steps[3:] == S).all())
    assert torch.equal(total[0], want["total"]) and bool((total[1:] == S).all())
    assert bool((ws[OP.WORKSPACE:] == S).all())


def test_wrapper_steps_an_optimiser_in_place():
    """adam_clip_step on the Adam of an ActorCriticRNN: the net's parameters and the optimiser's own state
    move as the reference says, twice in a row; the workspace is allocated once."""
    torch.manual_seed(5)
    net = I.ActorCriticRNN(6, [3, 4], 32, 32).cuda()
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=torch.tensor(LR, device="cuda"), eps=EPS, capturable=True)
    OP.init_adam_state(opt)
    ws = None
    for k in range(2):
        for p in params:
            p.grad = torch.randn_like(p)
        d = lambda ts: [t.detach().double().cpu() for t in ts]  # noqa: E731
        ref = OP.adam_clip_reference(d(params), d([p.grad for p in params]), d([opt.state[p]["exp_avg"] for p in params]),
                                     d([opt.state[p]["exp_avg_sq"] for p in params]), [float(k)] * len(params),
                                     float(np.float32(LR)), B1, B2, EPS, MAX_NORM)
        grads = [p.grad.clone() for p in params]
        total = OP.adam_clip_step(opt, MAX_NORM)
        assert total.shape == () and total.is_cuda
        got = dict(p=params, m=[opt.state[p]["exp_avg"] for p in params], v=[opt.state[p]["exp_avg_sq"] for p in params],
                   total=total)
        assert_outputs(f"wrapper step {k + 1}", got, dict(p=ref[0], m=ref[1], v=ref[2], total=float(ref[4])), LR)
        assert all(float(opt.state[p]["step"]) == k + 1.0 for p in params)
        assert all(torch.equal(p.grad, g) for p, g in zip(params, grads))
        ws = ws or opt._adam_clip_workspace.data_ptr()
        assert opt._adam_clip_workspace.data_ptr() == ws
    sd = opt.state_dict()
    assert sorted(sd["state"][0].keys()) == ["exp_avg", "exp_avg_sq", "step"] and float(sd["state"][0]["step"]) == 2.0
    # the state is what torch's own capturable step leaves: keys, dtypes, shapes, devices
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.Adam(twin, lr=torch.tensor(LR, device="cuda"), eps=EPS, capturable=True)
    fresh = torch.optim.Adam(params, lr=torch.tensor(LR, device="cuda"), eps=EPS, capturable=True)
    OP.init_adam_state(fresh)
    for q in twin:
        q.grad = torch.zeros_like(q)
    ref.step()
    for p, q in zip(params, twin):
        a, b = fresh.state[p], ref.state[q]
        assert list(a.keys()) == list(b.keys())
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
        assert float(a["step"]) == 0.0 and float(b["step"]) == 1.0 and not a["exp_avg"].any()


# ------------------------------------------------------------------ graphs
def test_graph_replay_is_the_eager_call_on_the_new_gradients():
    """The call captured in a graph (a serial chain of its two launches) and replayed after the
    contents of the gradient tensors were overwritten: bit for bit an eager call on those gradients."""
    first, _ = case("mixed4", 4 * MAX_NORM, 1000)
    second, _ = case("mixed4", MAX_NORM / 5, 1000)
    st = {k: [t.cuda() for t in first[k]] for k in ("p", "g", "m", "v")}
    steps = [torch.tensor(s, dtype=torch.float32, device="cuda") for s in first["steps"]]
    lr = torch.tensor(LR, dtype=torch.float32, device="cuda")
    ws = torch.empty(OP.WORKSPACE, dtype=torch.float64, device="cuda")
    total = torch.zeros((), dtype=torch.float32, device="cuda")
    n = len(st["p"])
    arr = (_lib.AdamTensor * n)(*[_lib.AdamTensor(*[_lib.ptr(st[k][i]) for k in ("p", "g", "m", "v")],
                                                  _lib.ptr(steps[i]), st["p"][i].numel()) for i in range(n)])

    def call():
        _lib.check(_lib.lib().hftlob_adam_clip(n, arr, _lib.ptr(lr), B1, B2, EPS, MAX_NORM, _lib.ptr(ws),
                                               _lib.ptr(total), _lib.stream_ptr()))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # a warm-up call before the capture
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k in ("p", "m", "v"):                            # the state back to the case's, the second case's gradients
        for t, s in zip(st[k], first[k]):
            t.copy_(s)
    for t, s in zip(st["g"], second["g"]):
        t.copy_(s)
    for t, s in zip(steps, first["steps"]):
        t.fill_(s)
    graph.replay()
    torch.cuda.synchronize()
    want = run_op(dict(first, g=second["g"]))
    for k in ("p", "m", "v"):
        assert all(torch.equal(a, b) for a, b in zip(st[k], want[k])), k
    assert all(torch.equal(a, b) for a, b in zip(steps, want["steps"])) and torch.equal(total, want["total"])
    assert not torch.equal(want["p"][0], run_op(first)["p"][0])


# ------------------------------------------------------------------ error codes
def test_error_codes_of_the_c_abi():
    L = _lib.lib()
    EINVAL, ENULL, ESHAPE = -1, -2, -3
    k = 64                                               # never dereferenced: the checks run before any launch

    def call(n=2, rows=None, lr=k, b1=B1, b2=B2, eps=EPS, max_norm=MAX_NORM, ws=k, arr=True):
        rows = rows if rows is not None else [(k, k, k, k, k, 5)] * max(n, 1)
        a = (_lib.AdamTensor * len(rows))(*[_lib.AdamTensor(*r) for r in rows]) if arr else None
        return L.hftlob_adam_clip(n, a, lr, b1, b2, eps, max_norm, ws, None, None)

    good = (k, k, k, k, k, 5)
    for kw, code in ((dict(n=0), ESHAPE), (dict(n=17, rows=[good] * 17), ESHAPE), (dict(n=-1), ESHAPE),
                     (dict(rows=[good, (k, k, k, k, k, 0)]), ESHAPE),
                     (dict(rows=[good, (None, k, k, k, k, 5)]), ENULL), (dict(rows=[good, (k, None, k, k, k, 5)]), ENULL),
                     (dict(rows=[good, (k, k, k, k, None, 5)]), ENULL), (dict(arr=False), ENULL),
                     (dict(lr=None), ENULL), (dict(ws=None), ENULL),
                     (dict(max_norm=0.0), EINVAL), (dict(max_norm=-1.0), EINVAL), (dict(max_norm=float("inf")), EINVAL),
                     (dict(max_norm=float("nan")), EINVAL), (dict(b1=1.0), EINVAL), (dict(b2=-0.1), EINVAL),
                     (dict(eps=-1e-5), EINVAL),
                     (dict(rows=[good, (k, k + 4, k, k, k, 5)]), EINVAL),      # g offset by one float
                     (dict(rows=[(k + 8, k, k, k, k, 5)], n=1), EINVAL)):
        assert call(**kw) == code, kw
        assert b"adam_clip" in L.hftlob_last_error()


# ------------------------------------------------------------------ the trainer
FQ = "2_player_fq_fqc"


@functools.lru_cache(maxsize=None)
def make_env():
    cfg = builtin_config(FQ)
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=False, persistent_outputs=True)


def config(**kw):
    return I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=32, FC_DIM_SIZE=32, UPDATE_EPOCHS=1,
                            NUM_MINIBATCHES=1, TOTAL_TIMESTEPS=64 * 8 * 4, **kw)


def state_of(tr, i):
    return [tr.opts[i].state[p] for p in tr.nets[i].parameters()]


@functools.lru_cache(maxsize=None)
def trainer_pair():
    """Two trainers of the same seed after one update, FUSED_OPT off and on; run once and shared."""
    runs = []
    for fused in (False, True):
        tr = I.IPPOTrainer(make_env(), config(CUDA_GRAPHS=False, FUSED_OPT=fused))
        before = [copy.deepcopy(n).cpu() for n in tr.nets]
        tr.update()
        runs.append((tr, before))
    torch.cuda.synchronize()
    return runs


def test_trainer_update_with_and_without_the_switch():
    (plain, before), (fused, _) = trainer_pair()
    assert fused.fused_opt and not plain.fused_opt
    assert all(g["capturable"] and torch.is_tensor(g["lr"]) and g["lr"].is_cuda for o in fused.opts for g in o.param_groups)
    for i in range(plain.n_types):
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(plain.buf[i], f.name), getattr(fused.buf[i], f.name)), (i, f.name)
        lr = plain.c["LR"][i]
        was = dict(before[i].named_parameters())
        for (name, p), q in zip(plain.nets[i].named_parameters(), fused.nets[i].parameters()):
            assert torch.allclose(q, p, rtol=1e-5, atol=lr * 2e-3), f"type {i}: {name} after one step"
            assert not torch.equal(p.cpu(), was[name]), name   # (and the step moved it)
        worst = 0.0
        for (name, _), a, b in zip(plain.nets[i].named_parameters(), state_of(plain, i), state_of(fused, i)):
            assert float(a["step"]) == 1.0 and float(b["step"]) == 1.0, name
            assert b["step"].is_cuda and b["step"].dtype == torch.float32
            for k in ("exp_avg", "exp_avg_sq"):
                w = over_bound(f"type {i} {name} {k}", b[k], a[k], float(a[k].double().abs().mean()))
                worst = max(worst, w)
                assert w <= 1.0, f"type {i}: {name} {k}: error / bound = {w}"
        print(f"type {i}: exp_avg, exp_avg_sq with the switch against without: largest error / bound = {worst:.4f}")


def test_trainer_graphs_on_and_off_give_the_same_bits_with_the_switch():
    """Four updates: the minibatch graph is captured at the third call, so they cover warm-up, capture
    and replay."""
    runs = []
    for graphs in (False, True):
        tr = I.IPPOTrainer(make_env(), config(CUDA_GRAPHS=graphs, FUSED_OPT=True))
        for _ in range(4):
            m = tr.update()
            assert all(np.isfinite(float(v)) for d in m["loss"] for v in d.values())
        runs.append(tr)
    torch.cuda.synchronize()
    eager, graph = runs
    assert graph.graphs and not eager.graphs
    assert [s["types"] for s in graph._steps] == [[i] for i in range(graph.n_types)]   # every type's own step
    assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in graph._steps)
    for i in range(eager.n_types):
        for (name, p), q in zip(eager.nets[i].named_parameters(), graph.nets[i].parameters()):
            assert torch.equal(p, q), f"type {i}: {name}"
        for a, b in zip(state_of(eager, i), state_of(graph, i)):
            assert float(a["step"]) == float(b["step"]) == 4.0


def test_checkpoints_move_between_runs_with_and_without_the_switch(tmp_path):
    for fused in (True, False):
        src = I.IPPOTrainer(make_env(), config(CUDA_GRAPHS=False, FUSED_OPT=fused))
        src.update()
        path = str(tmp_path / f"ck_{int(fused)}.pt")
        src.save_checkpoint(path)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert ck["format"] == I.CHECKPOINT_FORMAT
        assert sorted(ck["opts"][0]["state"][0].keys()) == ["exp_avg", "exp_avg_sq", "step"]
        dst = I.IPPOTrainer(make_env(), config(CUDA_GRAPHS=False, FUSED_OPT=not fused, SEED=3))
        dst.load_checkpoint(path)
        for i in range(src.n_types):
            for p, q in zip(src.nets[i].parameters(), dst.nets[i].parameters()):
                assert torch.equal(p, q)
            for a, b in zip(state_of(src, i), state_of(dst, i)):
                assert float(b["step"]) == 1.0 and b["step"].is_cuda == (not fused)
                assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        before = [p.clone() for p in dst.nets[0].parameters()]
        m = dst.update()                                 # the restored trainer goes on training
        assert all(np.isfinite(float(v)) for d in m["loss"] for v in d.values())
        assert all(float(s["step"]) == 2.0 for s in state_of(dst, 0))
        assert not any(torch.equal(p, q) for p, q in zip(before, dst.nets[0].parameters()))
