"""CALC_EVAL in the IPPO trainer on the GPU (the reference's ippo_rnn_JAXMARL.py:943-975): after every
update NUM_STEPS_EVAL sampled steps of the current nets in a separate eval env.  E = 16, NUM_STEPS = 8,
NUM_STEPS_EVAL = 6, H = FC = 64, two updates, FUSED_POLICY on so that no sampling reads torch's
generator; the minibatch steps and the second rollout run as captured graphs (the default)."""
import pytest
import torch

from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv
from hftlob.train import ippo as I

pytestmark = pytest.mark.gpu

FQ = "2_player_fq_fqc"
E, T, T_EVAL, SEED, UPDATES = 16, 8, 6, 2, 2


_DAYS = {}


def make_env(return_info, seed):
    cfg = builtin_config(FQ)
    w = cfg.world_config
    if seed not in _DAYS:   # generated once per seed
        _DAYS[seed] = generate_day(n_msgs=30_000, seed=seed, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=_DAYS[seed], return_info=return_info, persistent_outputs=True)


def config(**kw):
    return I.default_config(NUM_ENVS=E, NUM_STEPS=T, GRU_HIDDEN_DIM=64, FC_DIM_SIZE=64, TOTAL_TIMESTEPS=E * T * 4,
                            FUSED_POLICY=True, SEED=SEED, **kw)


@pytest.fixture(scope="module")
def eval_env():
    return make_env(True, seed=11)


@pytest.fixture(scope="module")
def runs(eval_env):
    """two updates with CALC_EVAL on and off; after each update of the run with it on, what
    evaluate_policy gives for the nets as they are then and the documented seed"""
    from oracle import ref_py as R
    on = I.IPPOTrainer(make_env(False, seed=4), config(CALC_EVAL=True, NUM_STEPS_EVAL=T_EVAL), eval_env=eval_env)
    off = I.IPPOTrainer(make_env(False, seed=4), config())
    metrics, again = [], []
    for u in range(UPDATES):
        metrics.append(on.update())
        off.update()
        seed_u = R.threefry2x32(0x65766C, SEED, 0, u)[0]     # words "evl", SEED; counter (rank 0, update u)
        assert on.eval_seed(u) == seed_u
        again.append(EV.evaluate_policy(eval_env, on.nets, E, T_EVAL, seed_u, greedy=False))
    torch.cuda.synchronize()
    return on, off, metrics, again


def test_training_is_untouched(runs):
    on, off, _, _ = runs
    assert on.calc_eval and not off.calc_eval and on.T_eval == T_EVAL
    for i, (a, b) in enumerate(zip(on.nets, off.nets)):
        for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(x, y), (i, k)
    for i, (oa, ob) in enumerate(zip(on.opts, off.opts)):
        sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
        assert sa.keys() == sb.keys() and len(sa) > 0
        for p in sa:
            for k in sa[p]:
                assert torch.equal(torch.as_tensor(sa[p][k]).cpu(), torch.as_tensor(sb[p][k]).cpu()), (i, p, k)
    for i, (a, b) in enumerate(zip(on.buf, off.buf)):
        for name in ("obs", "done", "global_done", "action", "value", "reward", "log_prob"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (i, name)
    assert torch.equal(on.rng, off.rng) and torch.equal(on.pol_rng, off.pol_rng)
    assert torch.equal(on.state.buf, off.state.buf)
    assert all(torch.equal(x, y) for x, y in zip(on.h, off.h))
    assert on.opt_count == off.opt_count and on.opt_count[0] > 0


def test_metrics_are_evaluate_policy_with_the_documented_seed(runs):
    on, _, metrics, again = runs
    for u, (m, ev) in enumerate(zip(metrics, again)):
        assert isinstance(m["eval"], EV.EvalStats)
        assert torch.equal(m["eval"].stats, ev.stats)
        assert len(m["avg_reward_eval"]) == 2
        for i in range(2):
            assert m["avg_reward_eval"][i] == ev.reward(i)["mean"], (u, i)
            assert m["eval"].steps(i) == E * T_EVAL
    assert on.eval_seed(0) != on.eval_seed(1)
    assert not torch.equal(metrics[0]["eval"].stats, metrics[1]["eval"].stats)
    # the training metrics are there as before
    assert set(metrics[0]) == {"loss", "avg_reward", "avg_reward_eval", "eval"}


def test_off_by_default_and_its_requirements(eval_env):
    env = make_env(False, seed=4)
    tr = I.IPPOTrainer(env, config(), eval_env=eval_env)
    assert not tr.calc_eval and I.default_config()["CALC_EVAL"] is False
    assert "avg_reward_eval" not in tr.update()
    with pytest.raises(ValueError, match="return_info=True"):
        I.IPPOTrainer(env, config(CALC_EVAL=True), eval_env=env)       # built without return_info
    with pytest.raises(ValueError, match="eval_env"):
        I.IPPOTrainer(env, config(CALC_EVAL=True))
    with pytest.raises(ValueError, match="CALC_EVAL"):
        I.IPPOTrainer(env, I.default_config(NUM_ENVS=E, NUM_STEPS=T, GRU_HIDDEN_DIM=32, FC_DIM_SIZE=64, CALC_EVAL=True),
                      eval_env=eval_env)
    assert I.IPPOTrainer(env, config(CALC_EVAL=True), eval_env=eval_env).T_eval == T   # NUM_STEPS_EVAL defaults to NUM_STEPS
