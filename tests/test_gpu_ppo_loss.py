"""The update's fused GAE and PPO loss on the GPU (hftlob_gae, hftlob_ppo_loss, hftlob.train.loss, the
learner's FUSED_LOSS switch).  GAE is held to the trainer's calculate_gae on the CPU bit for bit.  The
loss and its gradient are held to the float64 CPU restatement evaluated from the same float32 inputs:
the gradients per tensor within |got - ref| <= 1e-5 |ref| + 1e-5 max|ref| (tests/test_gpu_gru_scan.py;
exactly 0 where the reference is 0 everywhere), each scalar within 1e-5 (|ref| + m), m the float64
mean of the absolute values of the scalar's per-element terms (actor_loss is a mean that cancels to
about 0 when ratio is near 1, so a purely relative bound would mean nothing there).

The inputs are kept off the decision boundaries of the loss (the clip range of the ratio, the clip
range of the value, u^2 == c^2 for a clipped value) by redrawing offending elements from the fixed
seed: a float32 evaluation may not take the other side of a branch than the float64 reference."""
import copy
import dataclasses
import functools

import numpy as np
import pytest
import torch

from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.train import ippo as I
from hftlob.train import loss as LS

pytestmark = pytest.mark.gpu

EPS, VF, ENT = 0.2, 0.5, 0.01
GAMMAS = [(0.999999999, 0.85), (0.999, 0.9)]
NAMES = ("total", "value_loss", "actor_loss", "entropy", "approx_kl", "clip_frac")
R = LS.ROWS   # the elements one workgroup of the element pass covers
# (lead shape, nvec): one element; one short of, exactly and one past a workgroup; [T, B] input with a
# dead head group (K = 4 of widths 3, 16, 1, 5); many workgroups and more than one moment workgroup;
# every lane of every group live over three workgroups, the last with one element
CASES = [((1,), (10,)), ((63,), (13,)), ((64,), (16,)), ((65,), (1,)), ((3, 40), (3, 16, 1, 5)), ((5000,), (10,)),
         ((2 * R + 1,), (16, 16, 16, 16))]
IDS = [f"{'x'.join(map(str, s))}-{'_'.join(map(str, n))}" for s, n in CASES]
ARGS = ("logits", "values", "actions", "rb_value", "rb_log_prob", "adv", "targets")


def _elements(x, nvec):
    d = [x[k].double() if x[k].dtype == torch.float32 else x[k] for k in ARGS]
    return LS.ppo_loss_elements(*d, EPS, nvec)


def _offending(x, nvec):
    """The elements on a decision boundary, from the float64 reference (flat bool [N])."""
    e = _elements(x, nvec)
    ratio, dv, u, c = e["ratio"], e["dv"], e["u"], e["c"]
    u2, c2 = u * u, c * c
    bad = ((ratio - 1).abs() - EPS).abs() < 1e-3
    bad |= ((dv.abs() - EPS).abs() < 1e-3) & (dv != 0)
    bad |= ((u2 - c2).abs() < 1e-3 * torch.maximum(u2, c2)) & (dv.abs() > EPS)   # (v != vc: the value is clipped)
    return bad


@functools.lru_cache(maxsize=None)
def case(lead, nvec):
    """Float32 inputs and the float64 CPU reference of every output; computed once per case and not
    modified by the tests."""
    nvec = list(nvec)
    N = int(np.prod(lead))
    g = torch.Generator().manual_seed(1000 * N + 7 * sum(nvec) + len(nvec))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    x = dict(logits=2.0 * r(N, sum(nvec)), values=r(N),
             actions=torch.stack([torch.randint(0, n, (N,), generator=g) for n in nvec], -1).to(torch.int32),
             adv=3.0 * r(N) + 1.0, targets=r(N))
    x["rb_value"] = x["values"] + 0.3 * r(N)
    x["rb_value"][:3] = x["values"][:3]
    x["rb_log_prob"] = torch.zeros(N)
    logp = _elements(x, nvec)["logp"]                  # (float64, of the float32 logits)
    x["rb_log_prob"] = (logp + 0.2 * r(N).double()).float()
    for _ in range(100):
        bad = _offending(x, nvec)
        if not bad.any():
            break
        n_bad = int(bad.sum())
        x["rb_log_prob"][bad] = (logp[bad] + 0.2 * r(n_bad).double()).float()
        x["targets"][bad] = r(n_bad)
        keep = bad.clone()
        keep[:3] = False                               # the tie rows keep rb_value == values
        x["rb_value"][keep] = x["values"][keep] + 0.3 * r(int(keep.sum()))
    assert not _offending(x, nvec).any()
    assert torch.equal(x["rb_value"][:3], x["values"][:3])
    x = {k: v.reshape(*lead, *v.shape[1:]) for k, v in x.items()}
    d = [x[k].double() if x[k].dtype == torch.float32 else x[k] for k in ARGS]
    out, d_logits, d_values = LS.ppo_loss_reference(*d, EPS, VF, ENT, nvec)
    m = [float(t.abs().mean()) for t in LS.ppo_loss_elements(*d, EPS, nvec)["terms"]]
    m = dict(value_loss=0.5 * m[0], actor_loss=m[1], entropy=m[2], approx_kl=m[3], clip_frac=m[4])
    m["total"] = m["actor_loss"] + VF * m["value_loss"] + ENT * m["entropy"]
    return x, dict(out={k: float(v) for k, v in zip(NAMES, out)}, m=m, d_logits=d_logits, d_values=d_values)


def dev(x):
    return [x[k].cuda() for k in ARGS]


def assert_close(name, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert not got.any(), f"{name}: reference is 0 everywhere, got max |x| = {float(got.abs().max())}"
        return 0.0
    bound = 1e-5 * ref.abs() + 1e-5 * scale
    worst = float(((got - ref).abs() / bound).max())
    print(f"{name}: max error / bound = {worst:.4f}")
    assert float(((got - ref).abs() - bound).max()) <= 0.0, f"{name}: max error / bound = {worst}"
    return worst


def assert_scalars(label, got6, ref):
    """Each scalar within 1e-5 (|ref| + m); prints error over bound."""
    worst = 0.0
    for name, got in zip(NAMES, got6):
        bound = 1e-5 * (abs(ref["out"][name]) + ref["m"][name])
        err = abs(float(got) - ref["out"][name])
        if bound == 0.0:
            assert err == 0.0, f"{label} {name}: the reference and its terms are 0, got {float(got)}"
            continue
        print(f"{label} {name}: error / bound = {err / bound:.4f}")
        worst = max(worst, err / bound)
        assert err <= bound, f"{label} {name}: got {float(got)}, reference {ref['out'][name]}, error / bound {err / bound}"
    return worst


# ------------------------------------------------------------------ GAE
def gae_case(T, n):
    g = torch.Generator().manual_seed(100 * T + n)
    reward, value, last_val = (torch.randn(*s, generator=g) for s in ((T, n), (T, n), (n,)))
    done = torch.rand(T, n, generator=g) < 0.3
    done[T // 2] = True                                # one step with every done set
    assert last_val.any()
    return reward, value, done, last_val


@pytest.mark.parametrize("T,n", [(1, 1), (2, 63), (3, 64), (5, 65), (64, 130)])
def test_gae_is_calculate_gae_bit_for_bit(T, n):
    x = gae_case(T, n)
    c = [t.cuda() for t in x]
    for gamma, lam in GAMMAS:
        want = I.calculate_gae(*x, gamma, lam)        # on the CPU, float32
        adv, tgt = LS.gae(*c, gamma, lam)
        assert adv.dtype == torch.float32 and adv.shape == (T, n) and tgt.shape == (T, n)
        assert torch.equal(adv.cpu(), want[0]), (gamma, lam)
        assert torch.equal(tgt.cpu(), want[1]), (gamma, lam)
    as_bytes = LS.gae(c[0], c[1], c[2].to(torch.uint8) * 3, c[3], gamma, lam)   # done as bytes: non-zero is set
    assert torch.equal(as_bytes[0], adv) and torch.equal(as_bytes[1], tgt)


# ------------------------------------------------------------------ the loss against float64
@pytest.mark.parametrize("lead,nvec", CASES, ids=IDS)
def test_loss_and_gradient_match_float64(lead, nvec):
    x, ref = case(lead, nvec)
    out6, d_logits, d_values = LS.ppo_loss_op(*dev(x), EPS, VF, ENT, nvec)
    assert out6.shape == (6,) and d_logits.shape == x["logits"].shape and d_values.shape == x["values"].shape
    worst = assert_scalars("fused", out6.cpu(), ref)
    worst = max(worst, assert_close("d_logits", d_logits, ref["d_logits"]), assert_close("d_values", d_values, ref["d_values"]))
    print(f"fused: largest error / bound = {worst:.4f}")
    # the same figures for the float32 definition with autograd on the CPU: what any float32 code uses of the bound
    lg, v = x["logits"].clone().requires_grad_(True), x["values"].clone().requires_grad_(True)
    o = I.ppo_loss_multi(lg, v, x["actions"], x["rb_value"], x["rb_log_prob"], x["adv"], x["targets"], EPS, VF, ENT, nvec)
    o[0].backward()
    cpu = assert_scalars("float32 CPU", [t.detach() for t in o], ref)
    cpu = max(cpu, assert_close("float32 CPU d_logits", lg.grad, ref["d_logits"]),
              assert_close("float32 CPU d_values", v.grad, ref["d_values"]))
    print(f"float32 CPU: largest error / bound = {cpu:.4f}")


@pytest.mark.parametrize("lead,nvec", [CASES[0], CASES[4], CASES[5], CASES[6]], ids=[IDS[0], IDS[4], IDS[5], IDS[6]])
def test_two_calls_give_the_same_bits_and_forward_only_the_same_scalars(lead, nvec):
    x, _ = case(lead, nvec)
    c = dev(x)
    a = LS.ppo_loss_op(*c, EPS, VF, ENT, nvec)
    b = LS.ppo_loss_op(*c, EPS, VF, ENT, nvec)
    for name, s, t in zip(("out6", "d_logits", "d_values"), a, b):
        assert torch.equal(s, t), name
    fwd = LS.ppo_loss_op(*c, EPS, VF, ENT, nvec, grad=False)
    assert fwd[1] is None and fwd[2] is None and torch.equal(fwd[0], a[0])
    with torch.no_grad():                               # no input needs a gradient: the forward-only call
        out = LS.ppo_loss_fused(*c, EPS, VF, ENT, nvec)
    assert torch.equal(torch.stack(out), a[0])


def test_gradient_stores_stay_inside_their_tensors():
    """N = 65, nvec (3, 16, 1, 5): the second workgroup has one live element and every group dead lanes.
    The outputs are allocated with spare rows behind them, filled with a sentinel that must be
    intact afterwards (memory the test owns)."""
    from hftlob import _lib
    import ctypes as C
    nvec, N, PAD, S = [3, 16, 1, 5], 65, 64, -12345.0
    x, _ = case((3, 40), (3, 16, 1, 5))
    c = [t.reshape(120, *t.shape[2:])[:N].contiguous() for t in dev(x)]
    want = LS.ppo_loss_op(*c, EPS, VF, ENT, nvec)
    d_logits = torch.full((N + PAD, 25), S, dtype=torch.float32, device="cuda")
    d_values = torch.full((N + PAD,), S, dtype=torch.float32, device="cuda")
    out6 = torch.full((6 + PAD,), S, dtype=torch.float32, device="cuda")
    ws = torch.full((LS.workspace_doubles(N) + PAD,), S, dtype=torch.float64, device="cuda")
    p = _lib.ptr
    _lib.check(_lib.lib().hftlob_ppo_loss(N, 4, (C.c_int * 4)(*nvec), *[p(t) for t in c], EPS, VF, ENT, p(ws), p(out6),
                                          p(d_logits), p(d_values), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(d_logits[:N], want[1]) and torch.equal(d_values[:N], want[2]) and torch.equal(out6[:6], want[0])
    for name, t, n in (("d_logits", d_logits, N), ("d_values", d_values, N), ("out6", out6, 6),
                       ("workspace", ws, LS.workspace_doubles(N))):
        assert bool((t[n:] == S).all()), f"{name}: written past its end"


# ------------------------------------------------------------------ autograd and graphs
@pytest.mark.parametrize("lead,nvec", [CASES[4], CASES[5]], ids=[IDS[4], IDS[5]])
def test_autograd_hands_out_the_operators_gradients(lead, nvec):
    x, _ = case(lead, nvec)
    c = dev(x)
    _, d_logits, d_values = LS.ppo_loss_op(*c, EPS, VF, ENT, nvec)
    for factor in (1.0, 2.0):
        lg, v = c[0].clone().requires_grad_(True), c[1].clone().requires_grad_(True)
        out = LS.ppo_loss_fused(lg, v, *c[2:], EPS, VF, ENT, nvec)
        assert len(out) == 6 and out[0].requires_grad and not any(t.requires_grad for t in out[1:])
        (factor * out[0]).backward()
        assert torch.equal(lg.grad, factor * d_logits) and torch.equal(v.grad, factor * d_values)
        assert lg.grad.shape == x["logits"].shape


def test_graph_replay_is_the_eager_call():
    nvec = (10,)
    first, _ = case((5000,), nvec)
    g = torch.Generator().manual_seed(5)
    second = {k: v.clone() for k, v in first.items()}     # a second case: other logits, values and advantages
    second["logits"] = first["logits"] + 0.05 * torch.randn(5000, 10, generator=g)
    second["values"] = first["values"] + 0.05 * torch.randn(5000, generator=g)
    second["adv"] = first["adv"].flip(0).contiguous()
    st = dev(first)
    lg, v = st[0].requires_grad_(True), st[1].requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # a warm-up step before the capture
        LS.ppo_loss_fused(lg, v, *st[2:], EPS, VF, ENT, nvec)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    lg.grad = v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = LS.ppo_loss_fused(lg, v, *st[2:], EPS, VF, ENT, nvec)
        out[0].backward()
        stats = torch.stack([t.detach() for t in out])
    with torch.no_grad():
        for t, s in zip(st, dev(second)):
            t.copy_(s)
    graph.replay()
    torch.cuda.synchronize()
    want = LS.ppo_loss_op(*dev(second), EPS, VF, ENT, nvec)
    assert torch.equal(stats, want[0]) and torch.equal(lg.grad, want[1]) and torch.equal(v.grad, want[2])
    assert not torch.equal(want[0], LS.ppo_loss_op(*dev(first), EPS, VF, ENT, nvec)[0])


# ------------------------------------------------------------------ the trainer
FQ = "2_player_fq_fqc"


def make_env(multi):
    cfg = builtin_config(FQ)
    if multi:   # the Execution type on fixed_prices, n_actions = 3: a MultiDiscrete space, a multi-head net
        agents = dict(cfg.dict_of_agents_configs)
        agents["Execution"] = dataclasses.replace(agents["Execution"], action_space="fixed_prices", n_actions=3,
                                                  fixed_quant_value=11)
        cfg = dataclasses.replace(cfg, dict_of_agents_configs=agents)
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=False, persistent_outputs=True)


def config(**kw):
    return I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=32, FC_DIM_SIZE=32, UPDATE_EPOCHS=1,
                            NUM_MINIBATCHES=1, TOTAL_TIMESTEPS=64 * 8 * 4, **kw)


@functools.lru_cache(maxsize=None)
def trainer_pair(multi):
    """Two trainers of the same seed after one update, FUSED_LOSS off and on, each with a float64 CPU
    copy of its nets and its carries from before the update; run once per env and shared."""
    env = make_env(multi)
    runs = []
    for fused in (False, True):
        tr = I.IPPOTrainer(env, config(CUDA_GRAPHS=False, FUSED_LOSS=fused))
        before = [copy.deepcopy(n).double().cpu() for n in tr.nets]
        h0 = [h.double().cpu() for h in tr.h]
        runs.append((tr, tr.update(), before, h0))
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("multi", [False, True], ids=["discrete", "fixed_prices"])
def test_trainer_update_with_and_without_the_switch(multi):
    (plain, _, before, _), (fused, _, _, _) = trainer_pair(multi)
    assert fused.fused_loss and not plain.fused_loss
    assert any(len(n.heads) > 1 for n in fused.nets) == multi
    for i in range(plain.n_types):
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(plain.buf[i], f.name), getattr(fused.buf[i], f.name)), (i, f.name)
        for k in ("adv", "tgt", "h0"):
            assert torch.equal(plain._st[i][k], fused._st[i][k]), (i, k)
        lr = plain.c["LR"][i]
        was = dict(before[i].named_parameters())
        for (name, p), q in zip(plain.nets[i].named_parameters(), fused.nets[i].parameters()):
            assert torch.allclose(q, p, rtol=1e-5, atol=lr * 2e-3), f"type {i}: {name} after one step"
            assert not torch.equal(p.cpu(), was[name].float()), name   # (and the step moved it)


@pytest.mark.parametrize("multi", [False, True], ids=["discrete", "fixed_prices"])
def test_trainer_loss_statistics_with_and_without_the_switch(multi):
    """The update's loss statistics of the two trainers within the scalar bound 1e-5 (|ref| + m): ref the
    statistic without the switch, m from a float64 evaluation of the step's loss at the parameters
    before the update."""
    (plain, m_plain, before, h0), (_, m_fused, _, _) = trainer_pair(multi)
    for i in range(plain.n_types):
        b, st, net = plain.buf[i], plain._st[i], before[i]
        with torch.no_grad():
            logits, values = net(h0[i], b.obs.double().cpu(), b.done.cpu())
        m = [float(t.abs().mean()) for t in LS.ppo_loss_elements(
            logits, values, b.action.cpu().view(8, -1, len(net.heads)), b.value.double().cpu(),
            b.log_prob.double().cpu(), st["adv"].double().cpu(), st["tgt"].double().cpu(), 0.2, net.heads)["terms"]]
        m = dict(value_loss=0.5 * m[0], actor_loss=m[1], entropy=m[2], approx_kl=m[3], clip_frac=m[4])
        m["total"] = m["actor_loss"] + 0.5 * m["value_loss"] + 0.01 * m["entropy"]
        ref = dict(out={k.replace("total_loss", "total"): float(x) for k, x in m_plain["loss"][i].items()}, m=m)
        print(f"type {i}: statistics without the switch {ref['out']}, m {m}")
        assert_scalars(f"type {i}", [m_fused["loss"][i][k] for k in ("total_loss",) + NAMES[1:]], ref)


def test_trainer_in_graphs_with_the_switch():
    tr = I.IPPOTrainer(make_env(False), config(CUDA_GRAPHS=True, FUSED_LOSS=True))
    for _ in range(4):
        m = tr.update()
        assert all(np.isfinite(float(v)) for d in m["loss"] for v in d.values())
        assert all(np.isfinite(float(r)) for r in m["avg_reward"])
    assert [s["types"] for s in tr._steps] == [[i] for i in range(tr.n_types)]   # every type's own step
    assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in tr._steps)
