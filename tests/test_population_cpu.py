"""PopulationTrainer and the GROUPED_POLICY switch without a GPU: the construction errors, the command line's
parsing, and a population of three members against their three solo trainers on a CPU stand-in env whose rows
are independent (switches off, loop scans): every member must equal its solo run bit for bit, with one
``env.step`` of P x E rows per rollout step."""
import dataclasses

import numpy as np
import pytest
import torch

from hftlob.train import ippo as I
from hftlob.train import population as POP


class _Space:
    def __init__(self, n=None, shape=None):
        self.n, self.shape = n, shape


class _MAC:
    number_of_agents_per_type = [1, 2]


class RowEnv:
    """CPU stand-in with MARLEnv's interface whose rows are independent: an env's obs, reward and done are
    functions of its own key, its own step count and its own action words.  Type 0 is Discrete(3), type 1
    MultiDiscrete([2, 3]); the state is the envs' step counts."""
    device = torch.device("cpu")
    list_of_agents_configs = [object(), object()]
    multi_agent_config = _MAC()
    observation_spaces = [_Space(shape=(3,)), _Space(shape=(4,))]
    action_spaces = [_Space(n=3), _Space(n=[2, 3])]
    default_params = None

    def __init__(self):
        self.step_rows = []

    def split_keys(self, keys, n):
        k = keys.to(torch.int64)
        j = torch.arange(n, dtype=torch.int64)
        return ((k[:, None, :] * 1_000_003 + j[None, :, None] * 7919 + 17) % (2 ** 31)).to(torch.int32)

    @staticmethod
    def _obs(seed, n, d):
        """[E, n, d] floats in [-1, 1) from the per-env int64 seed."""
        i = torch.arange(n * d, dtype=torch.int64).view(1, n, d)
        return ((seed[:, None, None] * 2654435761 + i * 40503 + 12345) % 65536).float() / 32768.0 - 1.0

    def reset(self, keys, params):
        k = keys.to(torch.int64)
        seed = k[:, 0] * 31 + k[:, 1]
        return [self._obs(seed, 1, 3), self._obs(seed + 1, 2, 4)], torch.zeros(keys.shape[0], dtype=torch.int64)

    def step(self, keys, state, actions, params):
        E = keys.shape[0]
        self.step_rows.append(E)
        assert actions[0].shape == (E, 1) and actions[1].shape == (E, 2, 2)
        k, t = keys.to(torch.int64), state + 1
        a = actions[0].view(E).to(torch.int64) + 3 * actions[1].reshape(E, -1).to(torch.int64).sum(-1)
        seed = k[:, 0] * 31 + k[:, 1] * 17 + t * 13 + a * 7
        done = (seed % 5 == 0) | (t % 6 == 0)
        r0 = ((actions[0].view(E, 1) == 0).float() + (seed % 11)[:, None].float() / 11.0)
        r1 = (seed % 7)[:, None].float().repeat(1, 2) / 7.0 - actions[1].float().sum(-1) * 0.25
        dones = {"__all__": done, "agents": [done[:, None], done[:, None].repeat(1, 2)]}
        return [self._obs(seed, 1, 3), self._obs(seed + 1, 2, 4)], t, [r0, r1], dones, {}


def config(**kw):
    return I.default_config(**{**dict(NUM_ENVS=8, NUM_STEPS=6, GRU_HIDDEN_DIM=16, FC_DIM_SIZE=16, NUM_MINIBATCHES=2,
                                      UPDATE_EPOCHS=2, TOTAL_TIMESTEPS=8 * 6 * 10, CUDA_GRAPHS=False), **kw})


MEMBERS = [dict(SEED=3, LR=[3e-3, 1e-3], ENT_COEF=[0.01, 0.02], GAMMA=[0.99, 0.9]),
           dict(SEED=4, LR=[1e-3, 1e-3], ENT_COEF=[0.0, 0.05], GAMMA=[0.999, 0.95], GAE_LAMBDA=[0.8, 0.9]),
           dict(SEED=11, LR=[2e-3, 5e-4], ENT_COEF=[0.03, 0.01], GAMMA=[0.9, 0.99], ANNEAL_LR=[False, True],
                MAX_GRAD_NORM=[0.25, 1.0], VF_COEF=[0.25, 0.5], CLIP_EPS=0.1)]


def assert_member_equals_solo(m, solo, lm, ls):
    assert m.opt_count == solo.opt_count and m.updates_done == solo.updates_done
    assert torch.equal(m.gen.get_state(), solo.gen.get_state())
    assert torch.equal(m.rng, solo.rng)
    for i in range(solo.n_types):
        for (name, p), q in zip(m.nets[i].named_parameters(), solo.nets[i].parameters()):
            assert torch.equal(p, q), f"type {i}: {name}"
            sa, sb = m.opts[i].state[p], solo.opts[i].state[q]
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(torch.as_tensor(sa[key]), torch.as_tensor(sb[key])), f"type {i}: {name} {key}"
        for f in dataclasses.fields(I.Rollout):
            assert torch.equal(getattr(m.buf[i], f.name), getattr(solo.buf[i], f.name)), (i, f.name)
        assert torch.equal(m.h[i], solo.h[i]) and torch.equal(m.last_obs[i], solo.last_obs[i])
    for u, (da, db) in enumerate(zip(lm, ls)):
        for i, (x, y) in enumerate(zip(da["loss"], db["loss"])):
            for key in x:
                assert np.isfinite(float(x[key])) and torch.equal(x[key], y[key]), (u, i, key)
        for x, y in zip(da["avg_reward"], db["avg_reward"]):
            assert torch.equal(x, y)


def test_population_of_three_equals_the_three_solo_trainers():
    updates = 3
    solos = []
    for kw in MEMBERS:
        env = RowEnv()
        tr = I.IPPOTrainer(env, config(**kw))
        solos.append((tr, [tr.update() for _ in range(updates)]))
        assert env.step_rows == [8] * (6 * updates)
    env = RowEnv()
    pop = POP.PopulationTrainer(env, [config(**kw) for kw in MEMBERS])
    assert len(pop.members) == 3 and len(pop.pairs) == 6
    metrics = [pop.update() for _ in range(updates)]
    assert env.step_rows == [3 * 8] * (6 * updates)          # one env.step of P x E rows per rollout step
    assert all(isinstance(ms, list) and len(ms) == 3 for ms in metrics)
    for k, (solo, ls) in enumerate(solos):
        assert_member_equals_solo(pop.members[k], solo, [ms[k] for ms in metrics], ls)
    # the members do differ from each other (the comparison above is not of three equal runs)
    assert not torch.equal(pop.members[0].buf[0].reward, pop.members[1].buf[0].reward)


def test_member_checkpoint_is_a_solo_checkpoint(tmp_path):
    pop = POP.PopulationTrainer(RowEnv(), [config(**kw) for kw in MEMBERS[:2]])
    pop.update()
    path = str(tmp_path / "m1.pt")
    pop.members[1].save_checkpoint(path)
    solo = I.IPPOTrainer(RowEnv(), config(**MEMBERS[1]))
    solo.load_checkpoint(path)
    for a, b in zip(solo.nets, pop.members[1].nets):
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert solo.opt_count == pop.members[1].opt_count
    pop.members[0].load_checkpoint(path)                      # and back, into another member
    assert all(torch.equal(p, q) for p, q in zip(pop.members[0].nets[1].parameters(), solo.nets[1].parameters()))
    assert all(np.isfinite(float(v)) for m in pop.update() for d in m["loss"] for v in d.values())


# ------------------------------------------------------------------ construction errors
def test_grouped_policy_needs_fused_policy_and_a_gpu():
    with pytest.raises(ValueError, match="GROUPED_POLICY needs FUSED_POLICY"):
        I.IPPOTrainer(RowEnv(), config(GROUPED_POLICY=True))
    with pytest.raises(ValueError, match="needs a GPU device"):
        I.IPPOTrainer(RowEnv(), config(GROUPED_POLICY=True, FUSED_POLICY=True, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64))


@pytest.mark.parametrize("key, value", [("NUM_ENVS", 16), ("NUM_STEPS", 4), ("GRU_HIDDEN_DIM", 32), ("FC_DIM_SIZE", 32),
                                        ("UPDATE_EPOCHS", 1), ("NUM_MINIBATCHES", 4), ("CUDA_GRAPHS", True),
                                        ("FUSED_GRU", True), ("GROUPED_SCAN", True), ("FUSED_LOSS", True)])
def test_population_names_a_disagreeing_shared_key(key, value):
    with pytest.raises(ValueError, match=rf"agree on {key}\b"):
        POP.PopulationTrainer(RowEnv(), [config(SEED=1), config(SEED=2, **{key: value})])


def test_population_limits_the_nets_of_a_fused_launch():
    # 5 members x 2 agent types = 10 nets: more than one grouped launch takes
    with pytest.raises(ValueError, match=r"GROUPED_POLICY.*at most 8 nets.*5 x 2 = 10"):
        POP.check_configs([config(SEED=s, FUSED_POLICY=True, GROUPED_POLICY=True) for s in range(5)], 2, "cuda")
    with pytest.raises(ValueError, match=r"FUSED_GRU.*at most 8 nets.*5 x 2 = 10"):
        POP.check_configs([config(SEED=s, FUSED_GRU=True) for s in range(5)], 2, "cuda")
    POP.check_configs([config(SEED=s, FUSED_GRU=True) for s in range(4)], 2, "cuda")      # 8 nets fit
    POP.check_configs([config(SEED=s, FUSED_GRU=True) for s in range(5)], 2, "cpu")       # the loops have no limit
    POP.check_configs([config(SEED=s) for s in range(5)], 2, "cuda")


def test_population_refuses_what_is_out_of_scope():
    with pytest.raises(ValueError, match="CALC_EVAL is not supported in a population"):
        POP.PopulationTrainer(RowEnv(), [config(SEED=1), config(SEED=2, CALC_EVAL=True)])
    with pytest.raises(ValueError, match="different env configs"):
        POP.PopulationTrainer(RowEnv(), [config(SEED=1, ENV_CONFIG="2_player_fq_fqc"),
                                         config(SEED=2, ENV_CONFIG="3_player_fq_fqc_dir")])
    with pytest.raises(ValueError, match="different env configs"):
        POP.check_configs([config(SEED=1), config(SEED=2, AGENT_CONFIGS={"x": 1})], 2, "cpu")
    with pytest.raises(ValueError, match="world size of 2"):
        POP.check_configs([config(SEED=1)], 2, "cpu", world=2)
    with pytest.raises(ValueError, match="at least one config"):
        POP.check_configs([], 2, "cpu")


# ------------------------------------------------------------------ the command line
def test_seeds_and_overrides_parsing(tmp_path):
    assert POP.parse_seeds("2,3,4,5") == [2, 3, 4, 5] and POP.parse_seeds(" 7 ") == [7]
    for bad in ("", "2,x", "1.5"):
        with pytest.raises(ValueError, match="--seeds"):
            POP.parse_seeds(bad)
    path = tmp_path / "sweep.yaml"
    path.write_text("- {LR: [0.001, 0.002], ENT_COEF: 0.0}\n- {GAMMA: 0.9, SEED: 40}\n")
    ov = POP.load_overrides(str(path), 2)
    assert ov == [{"LR": [0.001, 0.002], "ENT_COEF": 0.0}, {"GAMMA": 0.9, "SEED": 40}]
    base = config()
    cs = POP.member_configs(base, [2, 3], ov)
    assert [c["SEED"] for c in cs] == [2, 40] and cs[0]["LR"] == [0.001, 0.002] and cs[1]["GAMMA"] == 0.9
    assert cs[1]["LR"] == base["LR"] and cs[1]["LR"] is not base["LR"]   # the members do not share the base's lists
    assert [c["SEED"] for c in POP.member_configs(base, [5, 6])] == [5, 6]
    with pytest.raises(ValueError, match="2 override dicts for 3 members"):
        POP.load_overrides(str(path), 3)
    path.write_text("- {NUM_ENVS: 8}\n")
    with pytest.raises(ValueError, match="overrides NUM_ENVS"):
        POP.load_overrides(str(path), 1)
    path.write_text("{LR: 1}\n")
    with pytest.raises(ValueError, match="YAML list"):
        POP.load_overrides(str(path), 1)
