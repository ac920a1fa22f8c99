"""The training diagnostics (TRAIN_DIAG) on the GPU: hftlob_rollout_diag and hftlob_world_tally against their torch
definitions bit for bit (the shapes of tests/test_train_diag_cpu.py: one element, both sides of one stripe, one
element past the most stripes of the base size), eager, repeated and replayed from a captured graph; the env's
``return_info="raw"`` mode against ``True``; and the trainer and a population with the switch: training is bit for
bit what it is without it, the diagnostics are ``reduce_steps`` over the steps the test cloned, and the captured
run's equal the eager run's."""
import dataclasses
import functools
import os

import pytest
import torch

from hftlob import _lib
from hftlob.config_io import builtin_config, load_config_from_file
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.evaluate import EVAL_WORDS, W_EPISODES, W_RUN_LEN, W_RUN_SUM, reduce_steps
from hftlob.train import diag as D
from hftlob.train import ippo as I
from hftlob.train import population as POP
from test_train_diag_cpu import BASE_LOSS, DIAG_HEADS, DIAG_SIZES, diag_case, info_records

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = _lib.DIAG_STRIPE_ROWS
HERE = os.path.dirname(os.path.abspath(__file__))


def on_gpu(case):
    buf, adv, target = case
    return tuple(x.to(DEV) for x in buf), adv.to(DEV), target.to(DEV)


# ------------------------------------------------------------------ hftlob_rollout_diag
@pytest.mark.parametrize("nvec", DIAG_HEADS, ids=["K1", "K4"])
@pytest.mark.parametrize("N", DIAG_SIZES)
def test_rollout_diag_equals_its_reference(N, nvec):
    case = diag_case(N, nvec)
    want = D.rollout_diag_reference(*case, nvec)           # (on the CPU: the same float64 loop, fewer launches)
    buf, adv, target = on_gpu(case)
    got = D.rollout_diag(buf, adv, target, nvec)
    out = torch.full((86,), -1.0, dtype=torch.float64, device=DEV)
    ws = torch.full((D.diag_workspace(N) + 3,), float("nan"), dtype=torch.float64, device=DEV)
    again = D.rollout_diag(buf, adv, target, nvec, out=out, workspace=ws)
    torch.cuda.synchronize()
    assert again is out and torch.equal(got, out)          # two calls, the same bits
    assert torch.equal(got.cpu(), want), (got.cpu() - want).abs().max()
    assert bool(torch.isnan(ws[-3:]).all())                # nothing past the workspace's size is written


def test_rollout_diag_replayed_from_a_graph():
    N, nvec = R + 1, [16, 3, 16, 1]
    buf, adv, target = on_gpu(diag_case(N, nvec, seed=2))
    out = torch.zeros(86, dtype=torch.float64, device=DEV)
    ws = torch.empty(D.diag_workspace(N), dtype=torch.float64, device=DEV)
    eager = D.rollout_diag(buf, adv, target, nvec).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D.rollout_diag(buf, adv, target, nvec, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.rollout_diag(buf, adv, target, nvec, out=out, workspace=ws)
    out.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    other = on_gpu(diag_case(N, nvec, seed=3))             # the graph reads the tensors it captured: new values
    for dst, src in zip(buf + (adv, target), other[0] + other[1:]):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, D.rollout_diag(buf, adv, target, nvec)) and not torch.equal(out, eager)


def test_rollout_diag_of_nothing_is_zero():
    e = torch.empty(0, device=DEV)
    buf = (torch.empty((0, 2), dtype=torch.int32, device=DEV), e, e, e, torch.empty(0, dtype=torch.bool, device=DEV))
    out = torch.full((86,), 7.0, dtype=torch.float64, device=DEV)
    D.rollout_diag(buf, e, e, [3, 4], out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))


def test_rollout_diag_refuses_bad_tensors():
    buf, adv, target = on_gpu(diag_case(8, [3]))
    with pytest.raises(ValueError, match="out must"):
        D.rollout_diag(buf, adv, target, [3], out=torch.zeros(86, device=DEV))
    with pytest.raises(ValueError, match="workspace must"):
        D.rollout_diag(buf, adv, target, [3], workspace=torch.zeros(85, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="is on"):
        D.rollout_diag(buf, adv.cpu(), target, [3])


# ------------------------------------------------------------------ hftlob_world_tally
@pytest.mark.parametrize("E, T", [(1, 1), (65, 3), (256, 2)])
def test_world_tally_equals_its_reference(E, T):
    info = info_records(T, E, 2, seed=E)
    more = info_records(T + 1, E, 2, seed=E + 1)
    want = D.world_tally_reference(info)
    got = D.world_tally(info.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and bool(want.any())
    again = D.world_tally(more.to(DEV), got)                # a second call continuing the first, in place
    torch.cuda.synchronize()
    assert again is got and torch.equal(got.cpu(), D.world_tally_reference(more, want))


# ------------------------------------------------------------------ the env and the trainer
@functools.lru_cache(maxsize=None)
def make_env(name, tag, info="raw"):
    """One MARLEnv per use: a captured rollout holds the env's persistent output buffers."""
    cfg = (load_config_from_file(os.path.join(HERE, "golden", "reference_env_configs", name)) if name.endswith(".json")
           else builtin_config(name))
    w = cfg.world_config
    day = generate_day(n_msgs=30_000, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=info, persistent_outputs=True), cfg


def test_raw_info_mode_equals_the_dict_mode():
    name, E = "2_player_fq_fqc", 64
    ea, _ = make_env(name, "raw mode", "raw")
    eb, _ = make_env(name, "dict mode", True)
    assert ea.return_info == "raw" and getattr(ea, "return_info", False)
    keys = torch.arange(2 * E, dtype=torch.int32, device=DEV).reshape(E, 2)
    (oa, sa), (ob, sb) = ea.reset(keys, ea.default_params), eb.reset(keys, eb.default_params)
    for t in range(4):
        k = keys + 1000 * (t + 1)
        acts = ea.sample_actions(k)
        oa, sa, ra, da, ia = ea.step(k, sa, acts, ea.default_params)
        ob, sb, rb, db, ib = eb.step(k, sb, acts, eb.default_params)
        torch.cuda.synchronize()
        assert ia == {} and set(ib) == {"world", "agents"}
        assert all(torch.equal(x, y) for x, y in zip(oa + ra + da["agents"], ob + rb + db["agents"]))
        assert torch.equal(da["__all__"], db["__all__"]) and torch.equal(sa.buf, sb.buf)
        assert torch.equal(ea.last_info_words, eb.last_info_words) and torch.equal(ea.last_rewards, eb.last_rewards)
        assert bool(ea.last_info_words.any())
    assert ea._out["obs_raw"] is None and ea._out["debug"] is None and ea._out["msgs"] is None
    with pytest.raises(ValueError, match="return_info"):
        MARLEnv(None, builtin_config(name), data=ea.data, return_info="words")


FUSED = dict(FUSED_GRU=True, FUSED_POLICY=True, GROUPED_POLICY=True, FUSED_LOSS=True, FUSED_OPT=True, GROUPED_SCAN=True,
             FUSED_WGRAD=True, FUSED_WGRAD_WIDE=True)
UPDATES, T, E = 3, 24, 64


def config(cfg, **kw):
    return I.default_config(**{**dict(NUM_ENVS=E, NUM_STEPS=T, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, UPDATE_EPOCHS=1,
                                      NUM_MINIBATCHES=2, TOTAL_TIMESTEPS=E * T * 8,
                                      NUM_AGENTS_PER_TYPE=cfg.number_of_agents_per_type), **kw})


def keep(m):
    return {"loss": [{k: v.clone() for k, v in d.items()} for d in m["loss"]],
            "avg_reward": [r.clone() for r in m["avg_reward"]], "diag": m.get("diag")}


def run(env, c, updates=UPDATES):
    tr = I.IPPOTrainer(env, c)
    return tr, [keep(tr.update()) for _ in range(updates)]


def assert_same_training(a, la, b, lb):
    assert a.opt_count == b.opt_count and torch.equal(a.gen.get_state(), b.gen.get_state()) and torch.equal(a.rng, b.rng)
    for i in range(a.n_types):
        for (name, p), q in zip(a.nets[i].named_parameters(), b.nets[i].parameters()):
            assert torch.equal(p, q), f"type {i}: {name}"
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(torch.as_tensor(a.opts[i].state[p][key]), torch.as_tensor(b.opts[i].state[q][key]))
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(a.buf[i], f.name), getattr(b.buf[i], f.name)), (i, f.name)
        assert torch.equal(a.h[i], b.h[i])
    assert len(la) == len(lb) > 0
    for ma, mb in zip(la, lb):
        assert all(torch.equal(x, y) for x, y in zip(ma["avg_reward"], mb["avg_reward"]))
        for x, y in zip(ma["loss"], mb["loss"]):
            assert all(torch.equal(x[k], y[k]) and bool(torch.isfinite(x[k])) for k in BASE_LOSS)


def assert_same_diag(la, lb):
    assert len(la) == len(lb) > 0
    for ma, mb in zip(la, lb):
        a, b = ma["diag"], mb["diag"]
        assert torch.equal(a.stats.stats, b.stats.stats) and torch.equal(a.wstats, b.wstats)
        assert all(torch.equal(x, y) for x, y in zip(a.words, b.words))
        for x, y in zip(ma["loss"], mb["loss"]):
            assert torch.equal(x["approx_kl_0"], y["approx_kl_0"]) and torch.equal(x["clip_frac_0"], y["clip_frac_0"])


@pytest.fixture(scope="module")
def eager_diag():
    """the eager run with the switch and no other: (trainer, its metrics, per update the (rewards, info words, global
    dones) of every step, cloned behind ``env.step``, and per update each type's reference words of the buffers)"""
    env, cfg = make_env("2_player_fq_fqc", "eager diag")
    rec, real = [], env.step

    def step(*a, **k):
        out = real(*a, **k)
        rec.append((env.last_rewards.clone(), env.last_info_words.clone(), out[3]["__all__"].clone()))
        return out

    env.step = step
    try:
        tr = I.IPPOTrainer(env, config(cfg, CUDA_GRAPHS=False, TRAIN_DIAG=True))
        ms, words = [], []
        for _ in range(UPDATES):
            ms.append(keep(tr.update()))
            words.append([D.rollout_diag_reference(tr.buf[i], tr._st[i]["adv"], tr._st[i]["tgt"], tr.nets[i].heads)
                          for i in range(tr.n_types)])
    finally:
        del env.step
    torch.cuda.synchronize()
    assert len(rec) == UPDATES * T                        # one recorded env.step per rollout step
    return tr, ms, [rec[u * T:(u + 1) * T] for u in range(UPDATES)], words


def test_eager_trainer_trains_the_same_with_the_switch(eager_diag):
    tr, ms, _, _ = eager_diag
    env, cfg = make_env("2_player_fq_fqc", "eager plain")
    plain, lp = run(env, config(cfg, CUDA_GRAPHS=False))
    torch.cuda.synchronize()
    assert all(m["diag"] is None and set(m["loss"][0]) == set(BASE_LOSS) for m in lp)
    assert_same_training(tr, ms, plain, lp)


def test_eager_diag_is_the_definition_over_the_cloned_steps(eager_diag):
    tr, ms, steps, words = eager_diag
    prev, later_dones = None, 0
    for u, (m, st) in enumerate(zip(ms, steps)):
        rew, info, done = (torch.stack(x) for x in zip(*st))
        carry = torch.zeros((E, 2, EVAL_WORDS), dtype=torch.float64, device=DEV)
        if prev is not None:
            carry[:, :, W_RUN_SUM], carry[:, :, W_RUN_LEN] = prev[:, :, W_RUN_SUM], prev[:, :, W_RUN_LEN]
        want = reduce_steps(rew, info, done, tr.env.layout, stats=carry)
        d = m["diag"]
        assert tuple(rew.shape) == (T, E, 2) and d.stats.steps(0) == E * T and bool(want.any())
        assert torch.equal(d.stats.stats, want)
        assert torch.equal(d.wstats, D.world_tally_reference(info))
        for i in range(tr.n_types):
            assert torch.equal(d.words[i], words[u][i]) and d.words[i][0] == T * E
            assert d.moments(i)["dones"] == int(done.sum()) and set(m["loss"][i]) == set(BASE_LOSS) | {
                "approx_kl_0", "clip_frac_0"}
        if u:
            later_dones += int(want[:, :, W_EPISODES].sum())
        prev = want
        s = d.summary()
        assert sum(s[f"agent_{tr.env.type_names[0]}/action_{a}"] for a in range(tr.nets[0].heads[0])) == \
            pytest.approx(100.0)
    # episodes end after the first update: their running sums and lengths were carried over an update's end
    assert later_dones > 0


def test_graph_run_equals_its_eager_run():
    """CUDA_GRAPHS and every fused switch: with and without TRAIN_DIAG the same training, and the captured run's
    diag against the eager run's.  The eager twin has the same fused switches: FUSED_POLICY draws the rollout's
    samples from its own key chain instead of torch's generator, so a run without it takes other actions and no
    diag of it can equal this one's."""
    env, cfg = make_env("2_player_fq_fqc", "graphs")
    plain, lp = run(env, config(cfg, CUDA_GRAPHS=True, **FUSED))
    tr, ld = run(env, config(cfg, CUDA_GRAPHS=True, TRAIN_DIAG=True, **FUSED))
    torch.cuda.synchronize()
    assert isinstance(tr._roll, torch.cuda.CUDAGraph) and tr.graphs
    assert_same_training(tr, ld, plain, lp)
    env2, _ = make_env("2_player_fq_fqc", "fused eager")
    eager, le = run(env2, config(cfg, CUDA_GRAPHS=False, TRAIN_DIAG=True, **FUSED))
    torch.cuda.synchronize()
    assert_same_training(tr, ld, eager, le)
    assert_same_diag(ld, le)
    assert len(ld) == UPDATES and all(m["diag"].stats.steps(0) == E * T for m in ld)
    assert any(m["diag"].stats.episodes(0) > 0 for m in ld[1:])


def test_multidiscrete_mean_quantities():
    env, cfg = make_env("exec_debug_fixed_price.json", "multi")
    tr, ms = run(env, config(cfg, CUDA_GRAPHS=False, TRAIN_DIAG=True, NUM_ENVS=16, NUM_STEPS=8,
                             TOTAL_TIMESTEPS=16 * 8 * 8), updates=2)
    torch.cuda.synchronize()
    assert tr.nets[0].nvec is not None
    s = ms[-1]["diag"].summary()
    name = env.type_names[0]
    act = tr.buf[0].action.reshape(-1, len(tr.nets[0].heads)).double()
    for k in range(act.shape[1]):
        assert s[f"agent_{name}/action_dim_{k}_mean_quant"] == float(act[:, k].mean())
    assert not any(key.startswith(f"agent_{name}/action_") and "dim" not in key for key in s)


def test_population_member_diag_equals_its_solo_run():
    members = [dict(SEED=2, LR=[2.5e-4, 1e-3]), dict(SEED=3, LR=[1e-3, 2.5e-4], GAMMA=[0.99, 0.9])]
    kw = dict(CUDA_GRAPHS=True, TRAIN_DIAG=True, NUM_ENVS=32, TOTAL_TIMESTEPS=32 * T * 8, **FUSED)
    env, cfg = make_env("2_player_fq_fqc", "solo of 32")
    solos = [run(env, config(cfg, **kw, **m), updates=2) for m in members]
    penv, _ = make_env("2_player_fq_fqc", "population of 2")
    pop = POP.PopulationTrainer(penv, [config(cfg, **kw, **m) for m in members])
    metrics = [[keep(m) for m in pop.update()] for _ in range(2)]
    torch.cuda.synchronize()
    assert pop._tally.stats.shape[0] == 64 and isinstance(pop._roll, torch.cuda.CUDAGraph)
    for k, (solo, ls) in enumerate(solos):
        lm = [ms[k] for ms in metrics]
        assert_same_training(pop.members[k], lm, solo, ls)
        assert_same_diag(lm, ls)
    assert not torch.equal(metrics[0][0]["diag"].stats.stats, metrics[0][1]["diag"].stats.stats)
