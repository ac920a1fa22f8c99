"""The update's fused GAE and PPO loss without a GPU: the torch restatements of hftlob_gae and
hftlob_ppo_loss (hftlob.train.loss) against the trainer's calculate_gae (bit for bit in float32) and
against autograd of ppo_loss_multi (float64), the exports and the C-ABI argument checks
(include/hftlob.h; dummy pointers that are never dereferenced), and the FUSED_LOSS switch on a CPU
device."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from hftlob import _lib
from hftlob.train import ippo as I
from hftlob.train import loss as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")
GAMMAS = [(0.999999999, 0.85), (0.999, 0.9)]       # the shipped (GAMMA, GAE_LAMBDA) pairs; the first gamma rounds to 1.0f


# ------------------------------------------------------------------ GAE
@pytest.mark.parametrize("T,n", [(1, 1), (7, 65)])
@pytest.mark.parametrize("gamma,lam", GAMMAS)
def test_gae_reference_is_calculate_gae_bit_for_bit(T, n, gamma, lam):
    g = torch.Generator().manual_seed(100 * T + n)
    reward, value, last_val = (torch.randn(*s, generator=g) for s in ((T, n), (T, n), (n,)))
    done = torch.rand(T, n, generator=g) < 0.3
    done[T // 2] = True                              # one step with every done set
    want = I.calculate_gae(reward, value, done, last_val, gamma, lam)
    got = LS.gae_reference(reward, value, done, last_val, gamma, lam)
    assert got[0].dtype == torch.float32 and last_val.any()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------ the loss
def loss_inputs(N, nvec, seed, dtype=torch.float64):
    """Inputs of N elements: adv far from mean 0, ratios on both sides of the clip range, and three
    rows with rb_value == values bit for bit (the ``maximum`` tie)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)  # noqa: E731
    logits, values = 2.0 * r(N, sum(nvec)), r(N)
    actions = torch.stack([torch.randint(0, n, (N,), generator=g) for n in nvec], -1).to(torch.int32)
    lp = sum(torch.log_softmax(x, -1).gather(-1, actions[:, k].long().unsqueeze(-1)).squeeze(-1)
             for k, x in enumerate(logits.split(list(nvec), -1)))
    rb_value = values + 0.3 * r(N)
    rb_value[:3] = values[:3]
    return dict(logits=logits, values=values, actions=actions, rb_value=rb_value, rb_log_prob=lp + 0.2 * r(N),
                adv=3.0 * r(N) + 1.0, targets=r(N))


@pytest.mark.parametrize("nvec", [[10], [1], [3, 16, 1, 5], [16, 16, 16, 16]], ids=str)
def test_loss_reference_is_autograd_of_ppo_loss_multi(nvec):
    # N a power of two: the definition's clip_frac is `.float().mean()`, a float32 mean in any type, and
    # count / 128 is the same number in float32 and in float64
    N, eps, vf, ent = 128, 0.2, 0.5, 0.01
    x = loss_inputs(N, nvec, 11 + len(nvec))
    assert torch.equal(x["rb_value"][:3], x["values"][:3])
    logits, values = x["logits"].clone().requires_grad_(True), x["values"].clone().requires_grad_(True)
    want = I.ppo_loss_multi(logits, values, x["actions"], x["rb_value"], x["rb_log_prob"], x["adv"], x["targets"], eps,
                            vf, ent, nvec)
    want[0].backward()
    out, d_logits, d_values = LS.ppo_loss_reference(x["logits"], x["values"], x["actions"], x["rb_value"],
                                                    x["rb_log_prob"], x["adv"], x["targets"], eps, vf, ent, nvec)
    assert len(out) == 6 and d_logits.shape == logits.shape and d_values.shape == values.shape
    for name, got, ref in [(f"out[{i}]", out[i], want[i].detach()) for i in range(6)] + \
                          [("d_logits", d_logits, logits.grad), ("d_values", d_values, values.grad)]:
        bound = 1e-10 * float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"{name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
    assert float(out[5]) > 0.0 and float(values.grad[:3].abs().min()) > 0.0   # clipped rows exist; the tie rows have a gradient


def test_loss_reference_takes_time_major_inputs():
    nvec, eps, vf, ent = [3, 4], 0.2, 0.5, 0.01
    x = loss_inputs(12, nvec, 5)
    flat = LS.ppo_loss_reference(*x.values(), eps, vf, ent, nvec)
    tb = {k: v.reshape(3, 4, *v.shape[1:]) for k, v in x.items()}
    out, d_logits, d_values = LS.ppo_loss_reference(*tb.values(), eps, vf, ent, nvec)
    assert d_logits.shape == (3, 4, 7) and d_values.shape == (3, 4)
    assert torch.equal(d_logits.reshape(12, 7), flat[1]) and all(torch.equal(a, b) for a, b in zip(out, flat[0]))


# ------------------------------------------------------------------ the C ABI
NAMES = ("hftlob_gae", "hftlob_ppo_loss")


def test_symbols_are_declared_listed_and_exported():
    src = open(HEADER).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is declared in include/hftlob.h"
        assert name in _lib.EXPORTS
        assert re.search(r"\sT\s+" + name + r"\s*$", syms, re.M), f"{name} is exported by the library"
    assert _lib.lib().hftlob_version() == 8


def test_gae_argument_checks_run_before_any_device_call():
    L = _lib.lib()
    k = C.c_void_p(64)   # never dereferenced: the checks run on the host before any device call
    EINVAL, ENULL = -1, -2

    def call(T=4, n=8, reward=k, value=k, done=k, last_val=k, adv=k, targets=k):
        return L.hftlob_gae(T, n, reward, value, done, last_val, 0.99, 0.9, adv, targets, None)

    for kw, code in ((dict(T=0), EINVAL), (dict(n=0), EINVAL), (dict(T=-1), EINVAL), (dict(reward=None), ENULL),
                     (dict(value=None), ENULL), (dict(done=None), ENULL), (dict(last_val=None), ENULL),
                     (dict(adv=None), ENULL), (dict(targets=None), ENULL)):
        assert call(**kw) == code, kw
        assert b"gae" in L.hftlob_last_error()


def test_ppo_loss_argument_checks_run_before_any_device_call():
    L = _lib.lib()
    k = C.c_void_p(64)
    EINVAL, ENULL = -1, -2
    names = ("logits", "values", "actions", "rb_value", "rb_log_prob", "adv", "targets", "workspace", "out6")

    def call(N=8, K=None, nvec=(3, 4), d_logits=k, d_values=k, **ptrs):
        nv = None if nvec is None else (C.c_int * max(len(nvec), 1))(*nvec)
        K = (0 if nvec is None else len(nvec)) if K is None else K
        p = {n: ptrs.get(n, k) for n in names}
        return L.hftlob_ppo_loss(N, K, nv, p["logits"], p["values"], p["actions"], p["rb_value"], p["rb_log_prob"],
                                 p["adv"], p["targets"], 0.2, 0.5, 0.01, p["workspace"], p["out6"], d_logits, d_values,
                                 None)

    cases = [(dict(N=0), EINVAL, b"N"), (dict(N=-3), EINVAL, b"N"), (dict(K=0), EINVAL, b"K"),
             (dict(K=5, nvec=(2,) * 5), EINVAL, b"K"), (dict(nvec=(3, 0)), EINVAL, b"nvec"),
             (dict(nvec=(17,)), EINVAL, b"nvec"), (dict(nvec=(3, 4, 5, 17)), EINVAL, b"nvec"),
             (dict(K=2, nvec=None), ENULL, b"nvec"),
             (dict(d_logits=None), EINVAL, b"d_logits"), (dict(d_values=None), EINVAL, b"d_values")]
    cases += [({n: None}, ENULL, b"null") for n in names]
    cases += [({n: None, "d_logits": None, "d_values": None}, ENULL, b"null") for n in ("logits", "out6")]
    for kw, code, word in cases:
        assert call(**kw) == code, kw
        assert word in L.hftlob_last_error(), (kw, L.hftlob_last_error())


def test_supported_head_sizes_and_workspace():
    ok = LS.ppo_loss_supported
    assert ok([10]) and ok([1]) and ok([16] * 4) and ok((3, 16, 1, 5))
    assert not ok([]) and not ok([2] * 5) and not ok([17]) and not ok([3, 0]) and not ok([16, 16, 16, 17])
    src = open(HEADER).read()
    assert int(re.search(r"#define HFTLOB_PPO_LOSS_ROWS (\d+)", src).group(1)) == LS.ROWS
    head = int(re.search(r"#define HFTLOB_PPO_LOSS_WS_HEAD (\d+)", src).group(1))
    row = int(re.search(r"#define HFTLOB_PPO_LOSS_WS_ROW (\d+)", src).group(1))
    for N, blocks in ((1, 1), (LS.ROWS, 1), (LS.ROWS + 1, 2), (65536, 65536 // LS.ROWS)):
        assert LS.workspace_doubles(N) == head + row * blocks


def test_fused_operators_refuse_cpu_tensors():
    x = loss_inputs(8, [3], 1, torch.float32)
    with pytest.raises(RuntimeError, match="device"):
        LS.ppo_loss_fused(x["logits"], x["values"], x["actions"], x["rb_value"], x["rb_log_prob"], x["adv"],
                          x["targets"], 0.2, 0.5, 0.01, [3])
    with pytest.raises(RuntimeError, match="device"):
        LS.gae(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.bool), torch.zeros(3), 0.99, 0.9)


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


def test_fused_loss_needs_a_gpu_device():
    assert I.default_config()["FUSED_LOSS"] is False
    tr = I.IPPOTrainer(FakeEnv(), I.default_config(**KW), device="cpu")
    assert tr.fused_loss is False
    with pytest.raises(ValueError, match="FUSED_LOSS needs a GPU device"):
        I.IPPOTrainer(FakeEnv(), I.default_config(**KW, FUSED_LOSS=True), device="cpu")
