"""IPPO-RNN on a MultiDiscrete action space on the GPU: 2_player_fq_fqc with the Execution type on
``fixed_prices`` (one quantity in [0, 11) per price level, 3 levels), through the learner's rollout
with FUSED_POLICY off and on, the captured graphs, the checkpoints and evaluate_policy.  16 envs,
8 steps, H = FC = 64, a 30,000-message synthetic day.  Tolerance where float32 paths are compared,
per tensor: |got - ref| <= 1e-5 |ref| + 1e-5 max|ref| (tests/test_gpu_policy_step.py)."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.train import ippo as I

pytestmark = pytest.mark.gpu

FQ = "2_player_fq_fqc"
N_MSGS = 30_000
K, Q = 3, 11


def assert_close(name, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert not got.any(), f"{name}: reference is 0 everywhere, got max |x| = {float(got.abs().max())}"
        return
    excess = (got - ref).abs() - (1e-5 * ref.abs() + 1e-5 * scale)
    worst = float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * scale)).max())
    print(f"{name}: max error / bound = {worst:.4f}")
    assert float(excess.max()) <= 0.0, f"{name}: max error / bound = {worst}"


def variant(cfg, type_name, **changes):
    """A copy of `cfg` with fields of one agent type replaced (configs are frozen dataclasses)."""
    agents = dict(cfg.dict_of_agents_configs)
    agents[type_name] = dataclasses.replace(agents[type_name], **changes)
    return dataclasses.replace(cfg, dict_of_agents_configs=agents)


def make_env(return_info):
    cfg = variant(builtin_config(FQ), "Execution", action_space="fixed_prices", n_actions=K, fixed_quant_value=Q)
    w = cfg.world_config
    day = generate_day(n_msgs=N_MSGS, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=return_info, persistent_outputs=True)


@pytest.fixture(scope="module")
def env():
    return make_env(False)


@pytest.fixture(scope="module")
def env_info():
    return make_env(True)


def types(env):
    """(the MarketMaking type's index, the Execution type's): the one Discrete and the one MultiDiscrete space"""
    exe = [i for i, sp in enumerate(env.action_spaces) if isinstance(sp.n, list)]
    assert len(exe) == 1 and len(env.action_spaces) == 2 and env.action_spaces[exe[0]].n == [Q] * K
    return 1 - exe[0], exe[0]


def config(**kw):
    return I.default_config(NUM_ENVS=16, NUM_STEPS=8, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, TOTAL_TIMESTEPS=16 * 8 * 4, **kw)


@pytest.mark.parametrize("fused", [False, True], ids=["torch", "fused"])
def test_rollout_buffers(env, fused):
    mm, exe = types(env)
    tr = I.IPPOTrainer(env, config(FUSED_POLICY=fused, CUDA_GRAPHS=False))
    assert tr.nets[mm].nvec is None and tr.nets[exe].nvec == [Q] * K
    h0 = [h.clone() for h in tr.h]
    tr.rollout()
    torch.cuda.synchronize()
    n = tr.n_actors[exe]
    b = tr.buf[exe]
    assert b.action.shape == (8, n, K) and b.action.dtype == torch.int32
    assert int(b.action.min()) >= 0 and int(b.action.max()) < Q
    assert tr.buf[mm].action.shape == (8, tr.n_actors[mm]) and tr.buf[mm].action.dtype == torch.int32
    assert int(tr.buf[mm].action.min()) >= 0 and int(tr.buf[mm].action.max()) < env.action_spaces[mm].n
    with torch.no_grad():
        logits, values = tr.nets[exe](h0[exe], b.obs, b.done)
    assert logits.shape == (8, n, K * Q)
    lp = sum(torch.log_softmax(lg, -1).gather(-1, b.action[..., k].long().unsqueeze(-1)).squeeze(-1)
             for k, lg in enumerate(logits.split([Q] * K, -1)))
    assert_close("log_prob", b.log_prob, lp)
    assert_close("value", b.value, values)
    # the freshly initialised heads are near uniform: 8 x 16 draws per head take more than one quantity,
    # and the heads do not copy each other
    assert all(len(torch.unique(b.action[..., k])) > 1 for k in range(K))
    assert not torch.equal(b.action[..., 0], b.action[..., 1])
    with torch.no_grad():   # the MarketMaking type's rows are its single head's
        lg_mm, v_mm = tr.nets[mm](h0[mm], tr.buf[mm].obs, tr.buf[mm].done)
    assert_close("log_prob[mm]", tr.buf[mm].log_prob,
                 torch.log_softmax(lg_mm, -1).gather(-1, tr.buf[mm].action.long().unsqueeze(-1)).squeeze(-1))
    assert_close("value[mm]", tr.buf[mm].value, v_mm)


def test_updates_with_everything_fused_in_graphs(env):
    tr = I.IPPOTrainer(env, config(CUDA_GRAPHS=True, FUSED_GRU=True, FUSED_POLICY=True))
    for _ in range(2):
        m = tr.update()
        for d in m["loss"]:
            assert all(np.isfinite(float(v)) for v in d.values())
    assert isinstance(tr._roll, torch.cuda.CUDAGraph)   # the rollout did not fall back to eager
    assert [s["types"] for s in tr._steps] == [[i] for i in range(tr.n_types)]   # every type's own step
    assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in tr._steps)


def test_updates_in_graphs_without_the_fused_policy(env):
    """Without FUSED_POLICY the multi-head type's draws are one torch.multinomial per head from the
    trainer's generator: the rollout and the minibatch steps are captured as for Discrete types."""
    tr = I.IPPOTrainer(env, config(CUDA_GRAPHS=True, FUSED_GRU=True))
    for _ in range(2):
        m = tr.update()
        for d in m["loss"]:
            assert all(np.isfinite(float(v)) for v in d.values())
    assert isinstance(tr._roll, torch.cuda.CUDAGraph)   # the rollout did not fall back to eager
    assert [s["types"] for s in tr._steps] == [[i] for i in range(tr.n_types)]   # every type's own step
    assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in tr._steps)
    b = tr.buf[types(env)[1]]
    assert b.action.shape == (8, tr.n_actors[types(env)[1]], K) and int(b.action.min()) >= 0 and int(b.action.max()) < Q


def _constant_nets(env, actions, margin=10.0, seed=0):
    """Nets whose actor heads ignore their input: w_a2 = 0 and b_a2 = +margin on the type's chosen
    action, in every head of a multi-head net."""
    torch.manual_seed(seed)
    nets = [I.ActorCriticRNN(env.observation_spaces[i].shape[0], env.action_spaces[i].n, 64, 64).cuda()
            for i in range(len(actions))]
    fixed = copy.deepcopy(nets)
    with torch.no_grad():
        for n, a in zip(fixed, actions):
            n.actor2.weight.zero_()
            n.actor2.bias.zero_()
            off = 0
            for width in (n.nvec or [n.actor2.out_features]):
                n.actor2.bias[off + a] = margin
                off += width
    return nets, fixed


def test_checkpoint_and_policy_evaluation(env, env_info, tmp_path):
    mm, exe = types(env)
    tr = I.IPPOTrainer(env, config(CUDA_GRAPHS=False, FUSED_POLICY=True))
    tr.update()
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    nets = I.load_policy(path, env_info, "cuda")
    assert nets[exe].nvec == [Q] * K and nets[mm].nvec is None
    for a, b in zip(tr.nets, nets):
        assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    E, T = 16, 12
    ev = EV.evaluate_policy(env_info, nets, E, T, 3, greedy=True)
    assert ev.steps(mm) == E * T and ev.steps(exe) == E * T
    assert np.isfinite(ev.reward(exe)["mean"])
    # constant-logit nets: every head prefers one quantity, which is the fixed-action evaluation bit for bit
    acts = [0, 0]
    acts[mm], acts[exe] = 4, 7
    _, fixed = _constant_nets(env_info, acts)
    want = EV.evaluate_fixed_actions(env_info, acts, E, T, 3)
    got = EV.evaluate_policy(env_info, fixed, E, T, 3, greedy=True)
    assert torch.equal(got.stats, want.stats)
    other = list(acts)
    other[exe] = 2
    assert not torch.equal(EV.evaluate_policy(env_info, _constant_nets(env_info, other)[1], E, T, 3).stats, want.stats)
