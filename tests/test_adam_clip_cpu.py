"""The update's fused clip and Adam step without a GPU (hftlob.train.optim, the learner's FUSED_OPT
switch): the torch restatement of hftlob_adam_clip against clip_grad_norm_ + torch.optim.Adam(eps 1e-5)
on the CPU, in float64 to rtol 1e-12 and in float32 within the operator's bound (per element
1e-5 (|ref| + scale): scale is lr for a parameter, the tensor's mean |ref| for exp_avg and exp_avg_sq;
total_norm within 1e-5 ref), over three consecutive steps with the clip active and inactive; the state
init_adam_state creates against what a capturable torch step leaves; and the argument checks."""
import copy

import pytest
import torch

from hftlob.train import ippo as I
from hftlob.train import optim as OP

LR, B1, B2, EPS, MAX_NORM = 2.5e-4, 0.9, 0.999, 1e-5, 0.5
SHAPES = [(5, 7), (7,), (33,), (1,)]


def tensors(dtype, grad_norm, seed):
    """Parameters and one gradient set of global norm ``grad_norm`` for every one of three steps."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(*s, generator=g, dtype=torch.float64).to(dtype) for s in SHAPES]
    grads = []
    for _ in range(3):
        gs = [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]
        n = torch.sqrt(sum((x ** 2).sum() for x in gs))
        grads.append([(x * (grad_norm / n)).to(dtype) for x in gs])
    return params, grads


def torch_steps(params, grads):
    """clip_grad_norm_ + Adam.step() on the CPU, one step per gradient set: per step (params, exp_avgs,
    exp_avg_sqs, steps, total_norm)."""
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()
        out.append(([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps],
                    [opt.state[p]["exp_avg_sq"].clone() for p in ps], [float(opt.state[p]["step"]) for p in ps],
                    total.clone()))
    return out


def reference_steps(params, grads):
    out = []
    p, m, v = params, [torch.zeros_like(x) for x in params], [torch.zeros_like(x) for x in params]
    s = [0.0] * len(params)
    for gs in grads:
        p, m, v, s, total = OP.adam_clip_reference(p, gs, m, v, s, LR, B1, B2, EPS, MAX_NORM)
        out.append((p, m, v, [float(x) for x in s], total))
    return out


@pytest.mark.parametrize("grad_norm", [2.0, 0.1], ids=["clip_active", "clip_inactive"])
def test_float64_reference_is_clip_grad_norm_and_adam(grad_norm):
    params, grads = tensors(torch.float64, grad_norm, seed=1)
    given = copy.deepcopy((params, grads))
    want, got = torch_steps(params, grads), reference_steps(params, grads)
    for a, b in zip(given[0] + sum(given[1], []), params + sum(grads, [])):
        assert torch.equal(a, b)                       # the reference modifies nothing it is given
    for k, (w, r) in enumerate(zip(want, got)):
        assert r[3] == w[3] == [k + 1.0] * len(SHAPES)
        torch.testing.assert_close(r[4], w[4], rtol=1e-12, atol=0)
        assert abs(float(w[4]) - grad_norm) < 1e-12 * grad_norm
        for name, ws, rs in zip(("p", "exp_avg", "exp_avg_sq"), w[:3], r[:3]):
            for i, (x, y) in enumerate(zip(ws, rs)):
                assert y.dtype == torch.float64
                torch.testing.assert_close(y, x, rtol=1e-12, atol=0, msg=lambda m: f"step {k} {name}[{i}]: {m}")
    if grad_norm > MAX_NORM:                            # the clip took part: exp_avg is that of the scaled gradient
        assert torch.allclose(got[0][1][0], grads[0][0] * (MAX_NORM / (grad_norm + 1e-6)) * (1 - B1), rtol=1e-12)
    else:
        assert torch.allclose(got[0][1][0], grads[0][0] * (1 - B1), rtol=1e-12)


def over_bound(got, ref, scale):
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (1e-5 * (ref.abs() + scale))).max())


@pytest.mark.parametrize("grad_norm", [2.0, 0.1], ids=["clip_active", "clip_inactive"])
def test_float32_reference_agrees_with_torch_in_float32(grad_norm):
    params, grads = tensors(torch.float32, grad_norm, seed=2)
    want, got = torch_steps(params, grads), reference_steps(params, grads)
    worst = 0.0
    for w, r in zip(want, got):
        assert r[4].dtype == torch.float32 and abs(float(r[4]) - float(w[4])) <= 1e-5 * float(w[4])
        for name, ws, rs in zip(("p", "exp_avg", "exp_avg_sq"), w[:3], r[:3]):
            for x, y in zip(ws, rs):
                assert y.dtype == torch.float32
                e = over_bound(y, x, LR if name == "p" else float(x.double().abs().mean()))
                worst = max(worst, e)
                assert e <= 1.0, f"{name}: error / bound = {e}"
    print(f"float32 reference against float32 torch: largest error / bound = {worst:.4f}")


def test_own_step_of_every_tensor():
    """Tensors whose steps differ: each gets the bias corrections of its own."""
    params, grads = tensors(torch.float64, 0.1, seed=3)
    zeros = [torch.zeros_like(x) for x in params]
    steps = [0.0, 5.0, 1000.0, 1.0]
    p, m, v, s, _ = OP.adam_clip_reference(params, grads[0], zeros, zeros, steps, LR, B1, B2, EPS, MAX_NORM)
    assert [float(x) for x in s] == [1.0, 6.0, 1001.0, 2.0]
    for i, st in enumerate(steps):
        one = OP.adam_clip_reference(params, grads[0], zeros, zeros, [st] * 4, LR, B1, B2, EPS, MAX_NORM)
        assert torch.equal(one[0][i], p[i])
    assert not torch.equal(OP.adam_clip_reference(params, grads[0], zeros, zeros, [0.0] * 4, LR, B1, B2, EPS,
                                                  MAX_NORM)[0][1], p[1])


# ------------------------------------------------------------------ the state
def test_init_adam_state_is_capturable_adams_first_state():
    def make():
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(*s)) for s in SHAPES]
        return ps, torch.optim.Adam(ps, lr=torch.tensor(LR), eps=EPS, capturable=True)

    ps, opt = make()
    OP.init_adam_state(opt)
    assert list(opt.state.keys()) == ps
    for p in ps:
        st = opt.state[p]
        assert list(st.keys()) == ["step", "exp_avg", "exp_avg_sq"]
        assert st["step"].dtype == torch.float32 and st["step"].shape == () and float(st["step"]) == 0.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == p.dtype and st[k].shape == p.shape and st[k].device == p.device and not st[k].any()
    qs, ref = make()
    for q in qs:
        q.grad = torch.zeros_like(q)
    try:   # torch creates the state, then refuses to step a capturable Adam on CPU tensors; the GPU test takes the step
        ref.step()
    except (RuntimeError, AssertionError):
        pass
    assert len(ref.state) == len(qs)
    for p, q in zip(ps, qs):
        a, b = opt.state[p], ref.state[q]
        assert list(a.keys()) == list(b.keys())
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
    # the state is the optimiser's own: it goes through state_dict and back, and a second call keeps it
    opt.state[ps[0]]["exp_avg"].fill_(3.0)
    opt.state[ps[0]]["step"].fill_(7.0)
    OP.init_adam_state(opt)
    assert float(opt.state[ps[0]]["step"]) == 7.0
    sd = copy.deepcopy(opt.state_dict())
    assert sorted(sd["state"].keys()) == list(range(len(SHAPES)))
    _, other = make()
    other.load_state_dict(sd)
    back = other.state_dict()
    for i in sd["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][k], sd["state"][i][k]) and back["state"][i][k].dtype == sd["state"][i][k].dtype
    assert float(back["state"][0]["step"]) == 7.0 and bool((back["state"][0]["exp_avg"] == 3.0).all())


# ------------------------------------------------------------------ validation
def test_supported_tensor_counts():
    assert OP.MAX_TENSORS == 16 and OP.CHUNK == 1024
    assert [OP.adam_clip_supported(n) for n in (0, 1, 14, 16, 17)] == [False, True, True, True, False]
    net = I.ActorCriticRNN(4, [3, 4], 16, 16)
    assert OP.adam_clip_supported(len(list(net.parameters()))) and len(list(net.parameters())) == 14


def _opt(n=3, dtype=torch.float32, grads=True):
    ps = [torch.nn.Parameter(torch.zeros(4, dtype=dtype)) for _ in range(n)]
    opt = torch.optim.Adam(ps, lr=torch.tensor(LR), eps=EPS, capturable=True)
    OP.init_adam_state(opt)
    if grads:
        for p in ps:
            p.grad = torch.ones_like(p)
    return ps, opt


def test_wrapper_refuses_what_the_operator_does_not_take():
    with pytest.raises(ValueError, match="parameter tensors"):
        OP.adam_clip_step(_opt(17)[1], MAX_NORM)
    ps, opt = _opt()
    ps[1].grad = None
    with pytest.raises(ValueError, match="no .grad"):
        OP.adam_clip_step(opt, MAX_NORM)
    with pytest.raises(ValueError, match="float32"):
        OP.adam_clip_step(_opt(dtype=torch.float64)[1], MAX_NORM)
    ps, opt = _opt()
    ps[0].grad = torch.ones(4, 2)[:, 0]                  # not contiguous
    with pytest.raises(ValueError, match="contiguous"):
        OP.adam_clip_step(opt, MAX_NORM)
    ps = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="lr"):          # the eager Adam's float lr
        OP.adam_clip_step(torch.optim.Adam(ps, lr=LR), MAX_NORM)
    with pytest.raises(ValueError, match="one param group"):
        OP.adam_clip_step(torch.optim.SGD(ps, lr=LR), MAX_NORM)
    with pytest.raises(RuntimeError, match="device"):    # everything in order, but on the CPU: no fall-back
        OP.adam_clip_step(_opt()[1], MAX_NORM)


def test_argument_checks_run_before_any_device_call():
    import os
    from hftlob import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    k = 64                                               # never dereferenced: the checks run on the host
    good = (k, k, k, k, k, 5)

    def call(n, rows, max_norm=MAX_NORM, b2=B2):
        arr = (_lib.AdamTensor * len(rows))(*[_lib.AdamTensor(*r) for r in rows])
        return L.hftlob_adam_clip(n, arr, k, B1, b2, EPS, max_norm, k, None, None)

    EINVAL, ENULL, ESHAPE = -1, -2, -3
    assert call(0, [good]) == ESHAPE and call(17, [good] * 17) == ESHAPE and call(1, [(k, k, k, k, k, 0)]) == ESHAPE
    assert call(2, [good, (None, k, k, k, k, 5)]) == ENULL and b"null" in L.hftlob_last_error()
    assert call(1, [good], max_norm=0.0) == EINVAL and call(1, [good], b2=1.0) == EINVAL
    assert call(1, [(k, k + 4, k, k, k, 5)]) == EINVAL and b"aligned" in L.hftlob_last_error()
    assert "hftlob_adam_clip" in _lib.EXPORTS


# ------------------------------------------------------------------ the trainer
class _Space:
    def __init__(self, n=None, shape=None):
        self.n, self.shape = n, shape


class _MAC:
    number_of_agents_per_type = [1, 2]


class FakeEnv:
    """CPU stand-in with MARLEnv's interface (tests/test_policy_multi_cpu.py): one Discrete and one
    MultiDiscrete agent type."""
    device = torch.device("cpu")
    list_of_agents_configs = [object(), object()]
    multi_agent_config = _MAC()
    observation_spaces = [_Space(shape=(3,)), _Space(shape=(4,))]
    action_spaces = [_Space(n=3), _Space(n=[3, 4])]
    default_params = None

    def split_keys(self, keys, n):
        k = keys.to(torch.int64)
        j = torch.arange(n, dtype=torch.int64)
        return ((k[:, None, :] * 1_000_003 + j[None, :, None] * 7919 + 17) % (2 ** 31)).to(torch.int32)

    def reset(self, keys, params):
        E = keys.shape[0]
        return [torch.zeros(E, 1, 3), torch.zeros(E, 2, 4)], None


KW = dict(NUM_ENVS=16, NUM_STEPS=6, FC_DIM_SIZE=16, GRU_HIDDEN_DIM=16, NUM_MINIBATCHES=2, UPDATE_EPOCHS=2,
          TOTAL_TIMESTEPS=16 * 6 * 4, SEED=0, CUDA_GRAPHS=False)


def test_fused_opt_needs_a_gpu_device():
    assert I.default_config()["FUSED_OPT"] is False
    tr = I.IPPOTrainer(FakeEnv(), I.default_config(**KW), device="cpu")
    assert tr.fused_opt is False
    assert not torch.is_tensor(tr.opts[0].param_groups[0]["lr"]) and len(tr.opts[0].state) == 0   # the eager Adam, as before
    with pytest.raises(ValueError, match="FUSED_OPT needs a GPU device"):
        I.IPPOTrainer(FakeEnv(), I.default_config(**KW, FUSED_OPT=True), device="cpu")
