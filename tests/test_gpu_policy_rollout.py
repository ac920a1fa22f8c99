"""The fused policy step in its two users on the GPU: the learner's rollout behind FUSED_POLICY
(hftlob.train.ippo) with its checkpoints, and hftlob.evaluate.evaluate_policy with its command line.
Env and day are those of test_trainer_updates_with_fused_gru_in_the_graph: 64 envs, 8 steps,
H = FC = 64.  Tolerance where float32 paths are compared, per tensor: |got - ref| <= 1e-5 |ref| +
1e-5 max|ref| (tests/test_gpu_gru_scan.py)."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.train import ippo as I
from hftlob.train import policy as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ = "2_player_fq_fqc"
N_MSGS = 30_000


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


def make_env(return_info):
    cfg = builtin_config(FQ)
    w = cfg.world_config
    day = generate_day(n_msgs=N_MSGS, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=return_info, persistent_outputs=True)


@pytest.fixture(scope="module")
def env():
    return make_env(False)


@pytest.fixture(scope="module")
def env_info():
    return make_env(True)


def config(**kw):
    return I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, TOTAL_TIMESTEPS=64 * 8 * 4, **kw)


def test_rollout_with_the_switch_on_and_off(env):
    on = I.IPPOTrainer(env, config(FUSED_POLICY=True, CUDA_GRAPHS=False))
    off = I.IPPOTrainer(env, config(CUDA_GRAPHS=False))
    assert on.fused_policy and not off.fused_policy
    assert torch.equal(on.reset_keys, off.reset_keys) and torch.equal(on.rng, off.rng)
    h0 = [h.clone() for h in on.h]
    pol0 = on.pol_rng.clone()
    on.rollout()
    off.rollout()
    torch.cuda.synchronize()
    assert torch.equal(on.rng, off.rng)                 # the env step keys do not depend on the switch
    assert not torch.equal(on.pol_rng, pol0)            # the sample keys have a chain of their own
    for i, net in enumerate(on.nets):
        b, n = on.buf[i], env.action_spaces[i].n
        assert b.action.dtype == torch.int32 and int(b.action.min()) >= 0 and int(b.action.max()) < n
        h, values, logps = h0[i], [], []
        with torch.no_grad():                           # net.step in torch over the saved obs and dones
            for t in range(on.T):
                h, logits, v = net.step(h, b.obs[t], b.done[t])
                values.append(v)
                logps.append(torch.log_softmax(logits, -1).gather(-1, b.action[t].long()[:, None]).squeeze(-1))
        assert_close(f"value[{i}]", b.value, torch.stack(values))
        assert_close(f"log_prob[{i}]", b.log_prob, torch.stack(logps))
        assert_close(f"h[{i}]", on.h[i], h)
        # the freshly initialised head is near uniform: a rollout of 512 samples takes more than one action
        assert len(torch.unique(b.action)) > 1


def test_updates_with_everything_fused_in_graphs(env):
    tr = I.IPPOTrainer(env, config(CUDA_GRAPHS=True, FUSED_GRU=True, FUSED_POLICY=True))
    for _ in range(3):
        m = tr.update()
        for d in m["loss"]:
            assert all(np.isfinite(float(v)) for v in d.values())
    assert isinstance(tr._roll, torch.cuda.CUDAGraph)   # the rollout did not fall back to eager
    assert [s["types"] for s in tr._steps] == [[i] for i in range(tr.n_types)]   # every type's own step
    assert all(isinstance(s["graph"], torch.cuda.CUDAGraph) for s in tr._steps)


def test_unsupported_size_raises(env):
    with pytest.raises(ValueError, match="FUSED_POLICY needs GRU_HIDDEN_DIM and FC_DIM_SIZE in"):
        I.IPPOTrainer(env, I.default_config(NUM_ENVS=64, NUM_STEPS=8, GRU_HIDDEN_DIM=32, FUSED_POLICY=True))


def _greedy(nets, obs, done, hs):
    return [P.policy_step(n, o, d, h.clone(), P.GREEDY, logits=True) for n, o, d, h in zip(nets, obs, done, hs)]


def test_checkpoint_round_trip(env, tmp_path):
    a = I.IPPOTrainer(env, config(CUDA_GRAPHS=False, FUSED_POLICY=True))
    a.update()
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path)
    b = I.IPPOTrainer(env, config(CUDA_GRAPHS=False, FUSED_POLICY=True, SEED=9))
    assert not torch.equal(a.nets[0].embed.weight, b.nets[0].embed.weight)
    b.load_checkpoint(path)
    assert b.opt_count == a.opt_count and a.opt_count[0] > 0
    for na, nb, oa, ob in zip(a.nets, b.nets, a.opts, b.opts):
        for (k, x), (_, y) in zip(na.state_dict().items(), nb.state_dict().items()):
            assert torch.equal(x, y), k
        sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
        assert sa.keys() == sb.keys() and len(sa) > 0
        for p in sa:
            for k in sa[p]:
                assert torch.equal(torch.as_tensor(sa[p][k]).cpu(), torch.as_tensor(sb[p][k]).cpu()), (p, k)
    nets = I.load_policy(path, env, "cuda")
    g = torch.Generator().manual_seed(2)
    obs = [torch.randn(20, n.embed.in_features, generator=g).cuda() for n in a.nets]
    hs = [torch.randn(20, 64, generator=g).cuda() for _ in a.nets]
    done = [(torch.arange(20) % 3 == 0).cuda() for _ in a.nets]
    for x, y in zip(_greedy(a.nets, obs, done, hs), _greedy(nets, obs, done, hs)):
        for name, u, v in zip(("h", "action", "log_prob", "value", "logits"), x, y):
            assert torch.equal(u, v), name


def _constant_nets(env, actions, margin=10.0, seed=0):
    """Nets whose actor head ignores its input: w_a2 = 0 and b_a2 = +margin on the type's chosen action."""
    torch.manual_seed(seed)
    nets = [I.ActorCriticRNN(env.observation_spaces[i].shape[0], env.action_spaces[i].n, 64, 64).cuda()
            for i in range(len(actions))]
    fixed = copy.deepcopy(nets)
    with torch.no_grad():
        for n, a in zip(fixed, actions):
            n.actor2.weight.zero_()
            n.actor2.bias.zero_()
            n.actor2.bias[a] = margin
    return nets, fixed


@pytest.mark.parametrize("E,T,seed,chunk", [(32, 40, 3, 16), (8, 70, 5, 32)])
def test_evaluate_policy_equals_fixed_actions(env_info, E, T, seed, chunk):
    """A policy that always takes a_t is the fixed-action evaluation bit for bit: the env keys are the
    same chain and reduce_steps is the kernel's reduction.  This config's episodes are 65 steps long,
    so the 70-step case is the one that crosses an auto-reset, where the actors' dones reset the
    carries."""
    acts = [4, 2]
    nets, fixed = _constant_nets(env_info, acts)
    want = EV.evaluate_fixed_actions(env_info, acts, E, T, seed, chunk=chunk)
    got = EV.evaluate_policy(env_info, fixed, E, T, seed, greedy=True, chunk=chunk)
    assert torch.equal(got.stats, want.stats)
    assert got.steps(0) == E * T
    if T > 65:
        assert got.total_dones() >= E
    # sampling takes a_t too once its margin beats every g[a] - g[a_t] drawn (checked on the CPU for the
    # keys used).  A margin of 10 does not at these counts: over the 32 x 40 x 23 draws of the first case
    # the largest difference is 13.74.  A float32 draw lies in [-4.47, 15.95] (u = tiny and u = 1 - 2^-23),
    # so 25 beats any difference the formula can produce.
    margin = 25.0
    gmax = _largest_noise(seed, E, T, [env_info.action_spaces[i].n for i in range(2)], acts)
    print(f"largest g[a] - g[a_t] over the keys used = {gmax:.3f}")
    assert gmax < margin
    samp = EV.evaluate_policy(env_info, _constant_nets(env_info, acts, margin)[1], E, T, seed, greedy=False,
                              chunk=chunk)
    assert torch.equal(samp.stats, want.stats)
    if T == 40:   # the untouched initial nets are near uniform: two seeds give different runs
        s1 = EV.evaluate_policy(env_info, nets, E, T, seed, greedy=False, chunk=chunk)
        s2 = EV.evaluate_policy(env_info, nets, E, T, seed + 1, greedy=False, chunk=chunk)
        assert not torch.equal(s1.stats, s2.stats)


def _largest_noise(seed, E, T, n_actions, acts):
    """On the CPU, over the policy keys of an evaluate_policy run (the oracle's split along the same
    chain): the largest g[a] - g[a_t], which is what the chosen action's margin has to beat."""
    from oracle import ref_py as R
    rng = R.split((0, seed), 2)[0]
    worst = -np.inf
    for _ in range(T):
        rng, act = R.split(rng, 2)
        rng = R.split(rng, 2)[0]
        for i, k in enumerate(R.split(act, len(n_actions))):
            g = P.gumbel_noise(np.array(k, np.uint32), E, n_actions[i])
            worst = max(worst, float((g - g[:, acts[i]:acts[i] + 1]).max()))
    return worst


def test_evaluate_policy_needs_info(env):
    nets, _ = _constant_nets(env, [0, 0])
    with pytest.raises(ValueError, match="return_info=True"):
        EV.evaluate_policy(env, nets, 4, 4, 0)


def test_command_line(env, tmp_path):
    tr = I.IPPOTrainer(env, config(CUDA_GRAPHS=False))
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    E, T = 8, 12
    run = subprocess.run([sys.executable, "-m", "hftlob.evaluate", "--env-config", FQ, "--checkpoint", path,
                          "--envs", str(E), "--steps", str(T), "--seed", "1", "--data-msgs", str(N_MSGS)],
                         capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=os.pathsep.join(
                             [os.path.join(ROOT, "jaxmarl-hft_amd")] + [p for p in sys.path if p])))
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["checkpoint"] == path and out["sample"] is False and out["envs"] == E and out["steps"] == T
    assert "total_dones" in out and len(out["types"]) == 2
    for t in range(2):
        assert set(out["types"][t]) == {"avg_reward", "std_reward", "steps", "episodes", "info", "episode_reward",
                                        "episode_length", "info_at_episode_end"}
        assert out["types"][t]["steps"] == E * T
