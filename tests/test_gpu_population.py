"""The learner's GROUPED_POLICY switch, PopulationTrainer and evaluate_policy(grouped=True) on the GPU, at the
tiny config of tests/test_gpu_gru_grouped.py with every fused switch on.  The nets, envs and optimisers of a
grouped launch, a joint step or a shared env batch are independent, so everything is compared bit for bit:
a trainer with the switch against one without, every member of a population against its solo trainer."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.evaluate import evaluate_policy
from hftlob.train import ippo as I
from hftlob.train import population as POP

pytestmark = pytest.mark.gpu
STEPS = 8   # NUM_STEPS


@functools.lru_cache(maxsize=None)
def make_env(name, batch="solo", info=False):
    """One MARLEnv per batch size it is stepped with: a captured rollout holds the env's persistent output
    buffers, and they are reallocated when the batch size changes."""
    cfg = builtin_config(name)
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=info, persistent_outputs=True), cfg


def config(cfg, **kw):
    return I.default_config(**{**dict(NUM_ENVS=16, NUM_STEPS=STEPS, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, UPDATE_EPOCHS=2,
                                      NUM_MINIBATCHES=2, TOTAL_TIMESTEPS=16 * STEPS * 8, FUSED_GRU=True,
                                      FUSED_POLICY=True, FUSED_LOSS=True, FUSED_OPT=True, FUSED_WGRAD=True,
                                      FUSED_WGRAD_WIDE=True,
                                      NUM_AGENTS_PER_TYPE=cfg.number_of_agents_per_type), **kw})


def keep(metrics):
    return [{k: v.clone() for k, v in d.items()} for d in metrics["loss"]]


def assert_same_training(a, la, b, lb, updates):
    assert a.opt_count == b.opt_count == [4 * updates] * a.n_types
    assert torch.equal(a.gen.get_state(), b.gen.get_state())
    assert torch.equal(a.rng, b.rng) and torch.equal(a.pol_rng, b.pol_rng)
    for i in range(a.n_types):
        for (name, p), q in zip(a.nets[i].named_parameters(), b.nets[i].parameters()):
            assert torch.equal(p, q), f"type {i}: {name}"
            sa, sb = a.opts[i].state[p], b.opts[i].state[q]
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sa[key], sb[key]), f"type {i}: {name} {key}"
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(a.buf[i], f.name), getattr(b.buf[i], f.name)), (i, f.name)
        assert torch.equal(a.h[i], b.h[i])
    assert len(la) == len(lb) > 0
    for u, (da, db) in enumerate(zip(la, lb)):
        for i, (x, y) in enumerate(zip(da, db)):
            for key in x:
                assert np.isfinite(float(x[key])) and torch.equal(x[key], y[key]), (u, i, key)


# ------------------------------------------------------------------ 6. the trainer switch
@pytest.mark.parametrize("name, updates, graphs", [("2_player_fq_fqc", 3, False), ("2_player_fq_fqc", 3, True),
                                                   ("3_player_fq_fqc_dir", 2, False), ("3_player_fq_fqc_dir", 2, True)])
def test_trainer_with_and_without_the_switch(name, updates, graphs, monkeypatch):
    env, cfg = make_env(name)
    calls = {"policy_step_net": 0, "policy_step_grouped": 0}

    def counted(fn, real):
        def wrapper(*a, **k):
            calls[fn] += 1
            return real(*a, **k)
        return wrapper

    for fn in calls:
        monkeypatch.setattr(I, fn, counted(fn, getattr(I, fn)))
    # a rollout's Python runs: every update when eager; under graphs the warm-up and the capture, then replays
    rollouts = ([1, 1] + [0] * (updates - 2)) if graphs else [1] * updates
    runs = []
    for on in (False, True):
        tr = I.IPPOTrainer(env, config(cfg, CUDA_GRAPHS=graphs, GROUPED_POLICY=on))
        assert tr.grouped_policy is on and tr.fused_policy and tr.graphs is graphs
        losses, counts = [], []
        for _ in range(updates):
            before = dict(calls)
            losses.append(keep(tr.update()))
            counts.append(tuple(calls[fn] - before[fn] for fn in ("policy_step_net", "policy_step_grouped")))
        if on:   # one grouped call per eager rollout step, and no per-net call
            assert counts == [(0, STEPS * r) for r in rollouts], counts
        else:
            assert counts == [(tr.n_types * STEPS * r, 0) for r in rollouts], counts
        runs.append((tr, losses))
    torch.cuda.synchronize()
    (a, la), (b, lb) = runs
    assert_same_training(a, la, b, lb, updates)
    if graphs:
        assert isinstance(b._roll, torch.cuda.CUDAGraph)


# ------------------------------------------------------------------ 7. a population against its solo trainers
MEMBERS = [dict(SEED=2, LR=[2.5e-4, 1e-3], ENT_COEF=[0.01, 0.02], GAMMA=[0.999, 0.99]),
           dict(SEED=3, LR=[1e-3, 2.5e-4], ENT_COEF=[0.0, 0.05], GAMMA=[0.99, 0.9]),
           dict(SEED=5, LR=[5e-4, 5e-4], ENT_COEF=[0.03, 0.01], GAMMA=[0.9, 0.999]),
           dict(SEED=8, LR=[3e-3, 1e-4], ENT_COEF=[0.02, 0.0], GAMMA=[0.95, 0.95])]


@pytest.mark.parametrize("name, P, graphs, solo_grouped_scan", [
    ("2_player_fq_fqc", 2, False, False), ("2_player_fq_fqc", 2, True, True), ("2_player_fq_fqc", 4, False, True),
    ("2_player_fq_fqc", 4, True, False), ("3_player_fq_fqc_dir", 2, False, False)])
def test_population_equals_its_solo_trainers(name, P, graphs, solo_grouped_scan, monkeypatch):
    updates = 3
    env, cfg = make_env(name)
    solos = []
    for kw in MEMBERS[:P]:
        tr = I.IPPOTrainer(env, config(cfg, CUDA_GRAPHS=graphs, GROUPED_POLICY=True, GROUPED_SCAN=solo_grouped_scan,
                                       **kw))
        solos.append((tr, [keep(tr.update()) for _ in range(updates)]))
    calls = {"policy_step_grouped": 0, "gru_scan_grouped": 0, "gru_scan": 0, "policy_step_net": 0}
    for fn in calls:
        def wrapper(*a, _fn=fn, _real=getattr(I, fn), **k):
            calls[_fn] += 1
            return _real(*a, **k)
        monkeypatch.setattr(I, fn, wrapper)
    penv, _ = make_env(name, batch=f"population of {P}")
    pop = POP.PopulationTrainer(penv, [config(cfg, CUDA_GRAPHS=graphs, GROUPED_POLICY=True, **kw) for kw in MEMBERS[:P]])
    assert pop.graphs is graphs and len(pop.pairs) == P * solos[0][0].n_types <= 8
    metrics = [pop.update() for _ in range(updates)]
    torch.cuda.synchronize()
    assert penv._out["obs"].shape[0] == P * 16                  # one env batch of P x E envs
    for k, (solo, ls) in enumerate(solos):
        assert_same_training(pop.members[k], [keep(ms[k]) for ms in metrics], solo, ls, updates)
        for ms, u in zip(metrics, range(updates)):
            assert all(torch.isfinite(r) for r in ms[k]["avg_reward"])
    # one grouped policy launch per eager rollout step and one grouped scan per eager joint step, for all the nets
    eager_rollouts, eager_steps = (2, 3) if graphs else (updates, 4 * updates)
    assert calls == {"policy_step_grouped": STEPS * eager_rollouts, "gru_scan_grouped": eager_steps, "gru_scan": 0,
                     "policy_step_net": 0}, calls
    if graphs:   # the rollout is one captured graph and the joint step one
        assert isinstance(pop._roll, torch.cuda.CUDAGraph) and isinstance(pop._joint["graph"], torch.cuda.CUDAGraph)
        assert all(m._roll is None and m._steps == [pop._joint] for m in pop.members)


# ------------------------------------------------------------------ 8. checkpoints
def test_member_checkpoint_loads_into_a_solo_trainer_and_back(tmp_path):
    name = "2_player_fq_fqc"
    env, cfg = make_env(name)
    penv, _ = make_env(name, batch="population of 2")
    kw = dict(CUDA_GRAPHS=True, GROUPED_POLICY=True)
    pop = POP.PopulationTrainer(penv, [config(cfg, **kw, **m) for m in MEMBERS[:2]])
    for _ in range(2):
        pop.update()
    path = str(tmp_path / "member1.pt")
    pop.members[1].save_checkpoint(path)
    # a solo trainer at the same point of the same run, then restored from the member's file: its next update
    # is the member's next update (same buffers-to-be: the envs and keys agree, the nets and optimisers are loaded)
    solo = I.IPPOTrainer(env, config(cfg, **kw, **MEMBERS[1]))
    for _ in range(2):
        solo.update()
    solo.load_checkpoint(path)
    pop.members[1].load_checkpoint(path)                         # and back into the population (captures again)
    assert pop._joint["graph"] is None
    ms, mp = keep(solo.update()), keep(pop.update()[1])
    torch.cuda.synchronize()
    assert_same_training(pop.members[1], [mp], solo, [ms], 3)
    assert I.load_policy(path, env)[0].hidden == 64


# ------------------------------------------------------------------ 9. evaluate_policy(grouped=True)
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("name", ["2_player_fq_fqc", "3_player_fq_fqc_dir"])
def test_grouped_evaluation_equals_the_per_type_launches(name, greedy):
    env, cfg = make_env(name, batch="eval", info=True)
    torch.manual_seed(3)
    nets = [I.ActorCriticRNN(env.observation_spaces[i].shape[0], env.action_spaces[i].n, 64, 64).to(env.device)
            for i in range(len(env.action_spaces))]
    a = evaluate_policy(env, nets, 8, 12, seed=5, greedy=greedy)
    b = evaluate_policy(env, nets, 8, 12, seed=5, greedy=greedy, grouped=True)
    torch.cuda.synchronize()
    assert torch.equal(a.stats, b.stats) and bool(a.stats.any())
