"""The grouped GRU scan without a GPU: the argument checks of hftlob.train.gru's grouped operators (they
raise before any launch), ActorCriticRNN.forward_grouped on the CPU (every net's scan is its loop) against
each net's own forward, and the learner's GROUPED_SCAN switch: the joint lockstep update on a two-type
stand-in env against the per-type update, bit for bit."""
import os
import re

import pytest
import torch

from hftlob import _lib
from hftlob.train import gru as G
from hftlob.train import ippo as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")


def group(T, B, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    return dict(gi=r(T, B, 3 * H), h0=r(B, H), done=torch.rand(T, B, generator=g) < 0.3, w_hh=r(3 * H, H) / H ** 0.5,
                b_hh=0.5 * r(3 * H))


def call(groups):
    return G.gru_scan_grouped(*([x[k] for x in groups] for k in ("gi", "h0", "done", "w_hh", "b_hh")))


def test_supported_and_abi_surface():
    assert G.MAX_GROUPS == 8
    for h in (64, 128, 256):
        assert G.gru_scan_grouped_supported(h, 1) and G.gru_scan_grouped_supported(h, 8)
        assert not G.gru_scan_grouped_supported(h, 0) and not G.gru_scan_grouped_supported(h, 9)
    assert not G.gru_scan_grouped_supported(32, 2) and not G.gru_scan_grouped_supported(96, 1)
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(hftlob_[a-z_]+)\s*\(", src))
    for name in ("hftlob_gru_scan_fwd_grouped", "hftlob_gru_scan_bwd_grouped"):
        assert name in declared and name in _lib.EXPORTS
    assert re.search(r"#define\s+HFTLOB_GRU_MAX_GROUPS\s+8\b", src)


def test_shape_disagreements_raise_before_any_launch():
    """CPU tensors: a launch attempt would raise RuntimeError (no device pointer), these raise ValueError first."""
    a = group(4, 3, 64)
    for bad, what in ((group(5, 3, 64), "same T and H"), (group(4, 3, 128), "same T and H")):
        with pytest.raises(ValueError, match=what):
            call([a, bad])
        with pytest.raises(ValueError, match=what):
            G.scan_forward_grouped([tuple(x[k] for k in ("gi", "h0", "done", "w_hh", "b_hh")) for x in (a, bad)])
    with pytest.raises(ValueError, match="1..8 groups, got 0"):
        call([])
    with pytest.raises(ValueError, match="1..8 groups, got 9"):
        call([a] * 9)
    with pytest.raises(ValueError, match="1..8 groups, got 9"):
        G.scan_backward_grouped([(a["h0"][None].expand(4, 3, 64),) * 2 + (None,) * 4] * 9)
    with pytest.raises(ValueError, match="1..8 groups, got 0"):
        G.scan_forward_grouped([])
    with pytest.raises(RuntimeError, match="device"):   # agreeing shapes reach the launch: a CPU tensor raises there
        call([a, group(4, 5, 64)])


def test_forward_grouped_on_the_cpu_equals_each_forward():
    torch.manual_seed(0)
    nets = [I.ActorCriticRNN(5, 4, 16, 8), I.ActorCriticRNN(7, [3, 2], 16, 8)]
    g = torch.Generator().manual_seed(1)
    T, Bs = 6, (5, 9)
    h0s = [torch.randn(B, 8, generator=g) for B in Bs]
    obss = [torch.randn(T, B, D, generator=g) for B, D in zip(Bs, (5, 7))]
    dones = [torch.rand(T, B, generator=g) < 0.3 for B in Bs]
    cot = [(torch.randn(T, B, A, generator=g), torch.randn(T, B, generator=g)) for B, A in zip(Bs, (4, 5))]

    def scalar(out, k):
        return (out[0] * cot[k][0]).sum() + (out[1] * cot[k][1]).sum()

    want = []
    for k, net in enumerate(nets):
        net.zero_grad(set_to_none=True)
        out = net(h0s[k], obss[k], dones[k])
        scalar(out, k).backward()
        want.append((out[0].detach(), out[1].detach(), [p.grad.clone() for p in net.parameters()]))
        net.zero_grad(set_to_none=True)
    outs = I.ActorCriticRNN.forward_grouped(nets, h0s, obss, dones)
    assert len(outs) == 2
    torch.autograd.backward([scalar(out, k) for k, out in enumerate(outs)])
    for k, net in enumerate(nets):
        assert torch.equal(outs[k][0], want[k][0]) and torch.equal(outs[k][1], want[k][1])
        for p, w in zip(net.parameters(), want[k][2]):
            assert torch.equal(p.grad, w)


class _Space:
    def __init__(self, n=None, shape=None):
        self.n, self.shape = n, shape


class _MAC:
    number_of_agents_per_type = [1, 3]


class TwoTypeEnv:
    """CPU stand-in with MARLEnv's interface: two agent types that differ in n_agents (1, 3) and obs size
    (3, 5); observations and rewards come from the env's own generator, seeded at reset."""
    device = torch.device("cpu")
    list_of_agents_configs = [object(), object()]
    multi_agent_config = _MAC()
    observation_spaces = [_Space(shape=(3,)), _Space(shape=(5,))]
    action_spaces = [_Space(n=3), _Space(n=[2, 3])]
    default_params = None

    def split_keys(self, keys, n):
        k = keys.to(torch.int64)
        j = torch.arange(n, dtype=torch.int64)
        return ((k[:, None, :] * 1_000_003 + j[None, :, None] * 7919 + 17) % (2 ** 31)).to(torch.int32)

    def reset(self, keys, params):
        E = keys.shape[0]
        self.g = torch.Generator().manual_seed(11)
        self.t = torch.zeros(E, dtype=torch.int64)
        return [torch.randn(E, 1, 3, generator=self.g), torch.randn(E, 3, 5, generator=self.g)], None

    def step(self, keys, state, actions, params):
        E = keys.shape[0]
        self.t += 1
        done = self.t % 3 == 0
        obs = [torch.randn(E, 1, 3, generator=self.g), torch.randn(E, 3, 5, generator=self.g)]
        rew = [(actions[0].view(E, 1) == 0).float(), torch.randn(E, 3, generator=self.g)]
        dones = {"__all__": done, "agents": [done[:, None], done[:, None].repeat(1, 3)]}
        return obs, state, rew, dones, {}


KW = dict(NUM_ENVS=8, NUM_STEPS=5, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=16, NUM_MINIBATCHES=2, UPDATE_EPOCHS=2,
          TOTAL_TIMESTEPS=8 * 5 * 6, LR=[3e-3, 1e-3], SEED=0, FUSED_GRU=True)


def test_switch_is_checked_at_construction():
    assert I.default_config()["GROUPED_SCAN"] is False
    with pytest.raises(ValueError, match="GROUPED_SCAN needs FUSED_GRU"):
        I.IPPOTrainer(TwoTypeEnv(), I.default_config(**{**KW, "FUSED_GRU": False}, GROUPED_SCAN=True))

    class _D:
        get_world_size = staticmethod(lambda: 2)
        get_rank = staticmethod(lambda: 0)
    with pytest.raises(ValueError, match="GROUPED_SCAN is single-process"):
        I.IPPOTrainer(TwoTypeEnv(), I.default_config(**KW, GROUPED_SCAN=True), dist=_D())

    class _Nine(TwoTypeEnv):
        list_of_agents_configs = [object()] * 9
    with pytest.raises(ValueError, match="GROUPED_SCAN needs <= 8 agent types, got 9"):
        I.IPPOTrainer(_Nine(), I.default_config(**KW, GROUPED_SCAN=True))
    assert not I.IPPOTrainer(TwoTypeEnv(), I.default_config(**KW)).grouped_scan


def _run(grouped, monkeypatch):
    calls = []
    real = I.ActorCriticRNN.forward_grouped
    monkeypatch.setattr(I.ActorCriticRNN, "forward_grouped",
                        staticmethod(lambda nets, *a, **k: (calls.append(len(nets)), real(nets, *a, **k))[1]))
    tr = I.IPPOTrainer(TwoTypeEnv(), I.default_config(**KW, GROUPED_SCAN=grouped))
    assert tr.grouped_scan is grouped and all(c for c in tr.c["ANNEAL_LR"])
    losses, per_update = [], []
    for _ in range(3):
        before = len(calls)
        m = tr.update()
        per_update.append(calls[before:])   # the number of nets of every forward_grouped call of this update
        losses.append([{k: v.clone() for k, v in d.items()} for d in m["loss"]])
        assert len(m["avg_reward"]) == 2
    return tr, losses, per_update


def test_joint_update_equals_the_per_type_update_bit_for_bit(monkeypatch):
    plain, l0, n0 = _run(False, monkeypatch)
    joint, l1, n1 = _run(True, monkeypatch)
    steps = KW["UPDATE_EPOCHS"] * KW["NUM_MINIBATCHES"]
    # (the last-value step of an update is net.step: it does not go through forward_grouped)
    assert n0 == [[1] * (plain.n_types * steps)] * 3   # every type's minibatch steps on their own, one net each
    assert n1 == [[joint.n_types] * steps] * 3         # the lockstep path: one call per step, all the nets
    assert plain.opt_count == joint.opt_count == [12, 12]
    assert torch.equal(plain.gen.get_state(), joint.gen.get_state())
    for a, b in zip(plain.nets, joint.nets):
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), n
    for a, b in zip(plain.opts, joint.opts):
        sa, sb = a.state_dict(), b.state_dict()
        assert sa["param_groups"] == sb["param_groups"]             # (the annealed lr among them)
        assert sa["state"].keys() == sb["state"].keys() and len(sa["state"]) > 0
        for k in sa["state"]:
            for name, v in sa["state"][k].items():
                w = sb["state"][k][name]
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(w)), (k, name)
    for u, (da, db) in enumerate(zip(l0, l1)):
        for i, (x, y) in enumerate(zip(da, db)):
            assert x.keys() == y.keys() and len(x) == 6
            for k in x:
                assert torch.equal(x[k], y[k]), (u, i, k)
    for a, b in zip(plain.buf, joint.buf):
        assert torch.equal(a.obs, b.obs) and torch.equal(a.action, b.action) and torch.equal(a.log_prob, b.log_prob)
