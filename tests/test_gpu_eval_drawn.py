"""The drawn baseline on the GPU: hftlob_draw_actions against its numpy definition
(hftlob.evaluate.draw_actions_reference), MARLEnv.rollout_eval_drawn / hftlob_env_rollout_eval_drawn
(k_env_rollout_eval_drawn: every env's wave draws its agents' actions at the top of each step) against
rollout_eval fed the same actions, bit for bit, and evaluate_baseline / evaluate_policy with Uniform
entries where they meet the fixed-action and per-step paths.

A device's float32 logarithm may round a last place differently from numpy's, so the comparisons with
the numpy definition hold the rows whose two largest allowed noises are at least GAP apart (the policy
step tests' rule and value); the comparisons between device paths are exact."""
import json

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv, split_keys
from hftlob.evaluate import Uniform
from hftlob.train import ippo as I
from hftlob.train import policy as P
from test_gpu_env import _day, _expect_launch, speed_test_config
from test_gpu_rollout_actions import NFIX, _same, _sized

pytestmark = pytest.mark.gpu
GAP = 1e-3
FQ = "2_player_fq_fqc"
ALL13 = (1 << 13) - 1
DRAW_CASES = [(1, 2, 0b11), (5, 10, 0b1000010010), (7, 13, ALL13), (3, 32, (1 << 31) | 1),
              (64, 13, ALL13), (65, 10, 0b0100000100)]


def _dev_key(words):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).cuda()


@pytest.mark.parametrize("B,A,mask", DRAW_CASES)
def test_draw_actions_against_the_definition(B, A, mask):
    """the first key (0, k), k < 64, whose smallest row gap is >= GAP: every row equals numpy's"""
    for k in range(64):
        want, gaps = EV.draw_actions_reference(np.array([0, k], np.uint32), B, A, mask)
        if gaps.min() >= GAP:
            break
    else:
        pytest.fail("no key (0, k), k < 64, with every row's gap >= GAP")
    got = EV.draw_actions(_dev_key([0, k]), B, A, mask)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B,)
    assert (got.cpu().numpy() == want).all(), (k, got.tolist(), want.tolist())
    out = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    assert EV.draw_actions(_dev_key([0, k]), B, A, mask, out=out[:B]) is not None
    assert (out[:B].cpu().numpy() == want).all() and int(out[B]) == -7, "nothing is written past n_actors"


def test_draw_actions_one_bit_and_bad_arguments():
    got = EV.draw_actions(_dev_key([5, 6]), 70, 10, 1 << 7)
    assert bool((got == 7).all())
    key, out = _dev_key([0, 1]), torch.full((4,), -7, dtype=torch.int32, device="cuda")
    R = _lib.lib().hftlob_draw_actions
    for args in ((0, 10, 3), (4, 0, 1), (4, 33, 3), (4, 10, 0), (4, 10, 1 << 10)):
        assert R(*args, key.data_ptr(), out.data_ptr(), None) == -1, args
    assert R(4, 10, 3, None, out.data_ptr(), None) == -1 and R(4, 10, 3, key.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all()), "a refused call launches nothing"
    for bad in ((0, 10, 3), (4, 33, 3), (4, 10, 0), (4, 10, 1 << 10)):
        with pytest.raises(ValueError):
            EV.draw_actions(key, *bad)
    with pytest.raises(ValueError, match="out"):
        EV.draw_actions(key, 4, 10, 3, out=out[:3])


# ------------------------------------------------------------------ the launch that draws
def draw_keys_numpy(seed, T, n_types):
    """the cases' draw keys, uint32 [T, n_types, 2]: split((0, seed), T * n_types) on the CPU"""
    return P.split_key(np.array([0, seed], np.uint32), T * n_types).reshape(T, n_types, 2)


def numpy_actions(dk, E, counts, sizes, masks):
    """the definition over all steps: (actions int32 [T, E, W], gaps float32 [T, E, W]), type i's actors
    env-major (b = e n_i + j) under dk[t, i]"""
    acts, gaps = [], []
    for t in range(dk.shape[0]):
        ra, rg = [], []
        for i, (n, A, m) in enumerate(zip(counts, sizes, masks)):
            a, g = EV.draw_actions_reference(dk[t, i], E * n, A, m)
            ra.append(a.reshape(E, n))
            rg.append(g.reshape(E, n))
        acts.append(np.concatenate(ra, axis=1))
        gaps.append(np.concatenate(rg, axis=1))
    return np.stack(acts), np.stack(gaps)


_CASES = {}


def drawn_case(tag, cfg, E, T, cuts, seed, entries=None):
    """One case, computed once and never modified: the drawn launch cut into `cuts` with stats carried
    and actions_out given, hftlob_draw_actions per step and type, and rollout_eval fed actions_out."""
    if tag in _CASES:
        return _CASES[tag]
    assert sum(cuts) == T
    env = MARLEnv(None, cfg, data=_day(cfg.world_config, 2_000_000))
    params = env.default_params
    counts = list(env.multi_agent_config.number_of_agents_per_type)
    sizes = [sp.n for sp in env.action_spaces]
    entries = entries or [Uniform.all()] * len(counts)
    masks = EV.draw_masks(env, EV.policy_entries(entries, len(counts)), fixed_too=True)
    k0 = torch.from_numpy(np.arange(2 * E, dtype=np.uint32).reshape(E, 2).view(np.int32) + 3).cuda()
    _, state = env.reset(k0, params)
    start = state.clone(env)
    keys = split_keys(k0, T).transpose(0, 1).contiguous()                         # [T, E, 2]
    dk_np = draw_keys_numpy(seed, T, len(counts))
    dk = _dev_key(dk_np)
    assert tuple(dk.shape) == (T, len(counts), 2)
    s = start.clone(env)
    acts = torch.full((T, E, env.action_words), -1, dtype=torch.int32, device="cuda")
    stats, t0 = None, 0
    for n in cuts:
        out = env.rollout_eval_drawn(keys[t0:t0 + n], s, dk[t0:t0 + n], masks, params, stats=stats,
                                     actions_out=acts[t0:t0 + n])
        assert out[1] is s and (stats is None or out[-1] is stats)
        stats, t0 = out[-1], t0 + n
    last = dict(obs=[x.clone() for x in out[0]], rew=[x.clone() for x in out[2]], done=out[3]["__all__"].clone(),
                dones=[x.clone() for x in out[3]["agents"]], info=env.last_info_words.clone())
    per_launch = torch.stack([torch.cat([EV.draw_actions(dk[t, i], E * n, A, m).view(E, n)
                                         for i, (n, A, m) in enumerate(zip(counts, sizes, masks))], dim=1)
                              for t in range(T)])
    s2 = start.clone(env)
    ref = env.rollout_eval(keys, s2, acts, params)
    ref_last = dict(obs=[x.clone() for x in ref[0]], rew=[x.clone() for x in ref[2]], done=ref[3]["__all__"].clone(),
                    dones=[x.clone() for x in ref[3]["agents"]], info=env.last_info_words.clone())
    torch.cuda.synchronize()
    _CASES[tag] = dict(env=env, params=params, start=start, keys=keys, dk=dk, dk_np=dk_np, masks=masks, counts=counts,
                       sizes=sizes, acts=acts, per_launch=per_launch, state=s.buf.clone(), stats=stats, last=last,
                       ref_state=s2.buf.clone(), ref_stats=ref[-1], ref_last=ref_last)
    return _CASES[tag]


def check_device_paths(V, T):
    """the bit-for-bit part of a case: the launch that draws against the other device paths"""
    assert V["acts"].dtype == torch.int32 and torch.equal(V["acts"], V["per_launch"]), \
        "actions_out vs hftlob_draw_actions per step and type"
    bad = torch.nonzero(V["state"] != V["ref_state"])
    assert bad.numel() == 0, f"end state vs rollout_eval on the drawn actions (env, word) {bad[:5].tolist()}"
    assert torch.equal(V["stats"], V["ref_stats"]), "stats vs rollout_eval on the drawn actions"
    a, b = V["last"], V["ref_last"]
    assert _same(a["obs"], b["obs"]) and _same(a["rew"], b["rew"]) and _same(a["dones"], b["dones"])
    assert bool((a["done"] == b["done"]).all()) and bool((a["info"] == b["info"]).all())
    assert bool((V["stats"][:, :, 0] == T).all())


def check_drawn_case(V, E, T, crosses=True):
    check_device_paths(V, T)
    if crosses:
        assert bool((V["stats"][:, :, 1] >= 1).all()), "every env crossed its episode end"
    # the numpy definition over all steps: the rows with a clear gap, which must be nearly all
    want, gaps = numpy_actions(V["dk_np"], E, V["counts"], V["sizes"], V["masks"])
    got = V["acts"].cpu().numpy()
    for i, A in enumerate(V["sizes"]):
        lo = sum(V["counts"][:i])
        assert ((got[:, :, lo:lo + V["counts"][i]] >= 0) & (got[:, :, lo:lo + V["counts"][i]] < A)).all()
    clear = gaps >= GAP
    share = 1.0 - clear.mean()
    print(f"rows left out (numpy gap < {GAP}): {int((~clear).sum())} of {clear.size} = {share:.4%}")
    assert share <= 0.01
    assert (got[clear] == want[clear]).all()
    assert len(np.unique(got)) > 1, "the draw moves"


def test_rollout_eval_drawn_two_player():
    """k_env_rollout_eval_drawn<2, 100, false, false>: E = 5, T = 70 in launches of 32, 32 and 6 steps
    with the stats carried, Uniform.all() for both types; every env crosses its 65-step episode end"""
    V = drawn_case("fq_fqc", builtin_config(FQ), 5, 70, (32, 32, 6), seed=11)
    _expect_launch(V["env"], NFIX)
    check_drawn_case(V, 5, 70)


def test_rollout_eval_drawn_three_types():
    V = drawn_case("3_player", builtin_config("3_player_fq_fqc_dir"), 5, 70, (32, 32, 6), seed=12)
    _expect_launch(V["env"], NFIX)
    assert len(V["counts"]) == 3
    check_drawn_case(V, 5, 70)


def test_rollout_eval_drawn_several_agents_per_type():
    """[5, 5] agents (the rows-in-trades kernel): an odd count, so a type's last pass draws one agent
    in both halves of the wave, and the second type's lanes start at 5"""
    V = drawn_case("rows_alias_32", speed_test_config([5, 5], 100), 5, 70, (32, 32, 6), seed=13)
    _expect_launch(V["env"], dict(slot_sets=2, nfix=100, random_cancel=0, rows_alias=1))
    assert V["counts"] == [5, 5] and V["env"].action_words == 10
    check_drawn_case(V, 5, 70)


def test_rollout_eval_drawn_general_kernel_and_a_mixed_mask():
    """k_env_rollout_eval_drawn<1, 0, false, false> (64 / 64 slots), E = 3, T = 8: a set of two
    actions for the first type and a fixed action (a mask of one bit) for the second"""
    V = drawn_case("sized_64_64", _sized(FQ, 64, 64), 3, 8, (5, 3), seed=14, entries=[Uniform([1, 4]), 2])
    _expect_launch(V["env"], dict(slot_sets=1, nfix=0, random_cancel=0, rows_alias=0))
    check_drawn_case(V, 3, 8, crosses=False)
    got = V["acts"].cpu().numpy()
    assert set(np.unique(got[:, :, 0])) == {1, 4} and (got[:, :, 1] == 2).all()


def test_rollout_eval_drawn_ranked_launch_and_one_step_launch():
    """E = 1025, T = 3 in launches of 2 steps and 1: the smallest launch whose waves rank their issue
    priority (after step 0 of the first launch), and a launch of the emitting step alone.  The device
    paths only: the numpy definition's share of clear rows is not known at this shape."""
    V = drawn_case("fq_fqc_1025", builtin_config(FQ), 1025, 3, (2, 1), seed=15)
    _expect_launch(V["env"], NFIX)
    check_device_paths(V, 3)


def test_rollout_eval_drawn_without_actions_out_and_bad_arguments():
    V = drawn_case("fq_fqc", builtin_config(FQ), 5, 70, (32, 32, 6), seed=11)
    env, params, keys, dk, masks = V["env"], V["params"], V["keys"], V["dk"], V["masks"]
    s = V["start"].clone(env)
    out = env.rollout_eval_drawn(keys, s, dk, masks, params)                  # one launch, no actions_out
    assert torch.equal(out[-1], V["stats"]) and bool((s.buf == V["state"]).all())
    s = V["start"].clone(env)
    stats = torch.full((5, env.num_agents, 106), 3.0, dtype=torch.float64, device="cuda")
    acts = torch.zeros((70, 5, env.action_words), dtype=torch.int32, device="cuda")
    bad = [dict(draw_keys=dk[:-1]), dict(draw_keys=dk.cpu()), dict(draw_keys=dk[:, :1]), dict(draw_keys=dk.long()),
           dict(allowed=masks[:1]), dict(allowed=[0, 1]), dict(allowed=[1, 1 << 31]), dict(allowed=[-1, 1]),
           dict(actions_out=acts[:, :4]), dict(actions_out=acts.long()), dict(actions_out=acts.cpu()),
           dict(stats=stats.float()), dict(key=keys[:, :4])]
    for kw in bad:
        a = dict(key=keys, draw_keys=dk, allowed=masks, stats=stats, actions_out=None)
        a.update(kw)
        with pytest.raises((ValueError, _lib.HftlobError)):
            env.rollout_eval_drawn(a["key"], s, a["draw_keys"], a["allowed"], params, stats=a["stats"],
                                   actions_out=a["actions_out"])
    torch.cuda.synchronize()
    assert bool((s.buf == V["start"].buf).all()) and bool((stats == 3.0).all()), "a refused call launches nothing"
    legacy = MARLEnv(None, builtin_config(FQ), data=_day(builtin_config(FQ).world_config, 2_000_000),
                     prng_partitionable=False)
    _, ls = legacy.reset(keys[0], legacy.default_params)
    with pytest.raises(_lib.HftlobError, match="prng_partitionable"):
        legacy.rollout_eval_drawn(keys, ls, dk, masks, legacy.default_params)


# ------------------------------------------------------------------ where the paths meet
N_MSGS = 30_000


@pytest.fixture(scope="module")
def env():
    cfg = builtin_config(FQ)
    w = cfg.world_config
    day = generate_day(n_msgs=N_MSGS, seed=4, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, return_info=True, persistent_outputs=True)


def test_one_bit_sets_are_fixed_actions(env):
    """evaluate_baseline with Uniform([4]) and a plain 2: evaluate_fixed_actions([4, 2]) bit for bit"""
    want = EV.evaluate_fixed_actions(env, [4, 2], 6, 70, 9)
    got = EV.evaluate_baseline(env, [Uniform([4]), 2], 6, 70, 9)
    assert torch.equal(got.stats, want.stats)
    got = EV.evaluate_baseline(env, [[4], Uniform([2])], 6, 70, 9, chunk=32)
    assert torch.equal(got.stats, want.stats) and got.total_dones() >= 6


def test_persistent_launch_meets_the_per_step_path(env):
    """the same drawn entries through evaluate_baseline (the draw inside the env launch) and
    evaluate_policy (one hftlob_draw_actions, env.step and tally launch per step)"""
    entries = [Uniform([1, 4]), Uniform.all()]
    a = EV.evaluate_baseline(env, entries, 6, 70, 21)
    b = EV.evaluate_policy(env, entries, 6, 70, 21)
    assert torch.equal(a.stats, b.stats)
    assert a.steps(0) == 6 * 70 and a.total_dones() >= 6
    c = EV.evaluate_baseline(env, entries, 6, 70, 22)
    f = EV.evaluate_fixed_actions(env, [1, 0], 6, 70, 21)
    assert not torch.equal(a.stats, c.stats) and not torch.equal(a.stats, f.stats), "the draw moves with the seed"


def test_the_draw_leaves_the_learned_chain_alone(env, monkeypatch):
    """sampled [net, Uniform([0, 2])] and [net, 2]: the learned type's first-step samples are the same
    (its key is split(act, n_types)[0] whatever the other entry is, and the draw touches no carry)"""
    torch.manual_seed(0)
    net = I.ActorCriticRNN(env.observation_spaces[0].shape[0], env.action_spaces[0].n, 64, 64).cuda()
    seen = []
    real = P.policy_step_net

    def recorder(*args, **kw):
        out = real(*args, **kw)
        seen.append(out[1].clone())
        return out

    monkeypatch.setattr(P, "policy_step_net", recorder)
    EV.evaluate_policy(env, [net, Uniform([0, 2])], 6, 2, 31, greedy=False)
    with_draw = [x.cpu() for x in seen]
    del seen[:]
    EV.evaluate_policy(env, [net, 2], 6, 2, 31, greedy=False)
    fixed = [x.cpu() for x in seen]
    assert len(with_draw) == len(fixed) == 2
    assert torch.equal(with_draw[0], fixed[0]), "the first step's samples"
    assert len(torch.unique(with_draw[0])) > 1, "a fresh net's samples spread"
    mixed = EV.evaluate_policy(env, [net, Uniform([2])], 6, 8, 31, greedy=False)
    assert torch.equal(mixed.stats, EV.evaluate_policy(env, [net, 2], 6, 8, 31, greedy=False).stats)


def test_command_line_in_process(env, capsys):
    """--uniform-actions with one-action sets is --fixed-actions' evaluation"""
    assert EV.main(["--env-config", FQ, "--uniform-actions", "4,2", "--envs", "6", "--steps", "20", "--seed", "9",
                    "--data-msgs", str(N_MSGS)]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    cfg = builtin_config(FQ)
    w = cfg.world_config
    day = generate_day(n_msgs=N_MSGS, snap_every=w.n_data_msg_per_step * w.start_resolution)
    e2 = MARLEnv(None, cfg, data=day, device="cuda:0", return_info=False, persistent_outputs=True)
    want = EV.evaluate_fixed_actions(e2, [4, 2], 6, 20, 9).summary()
    assert out["uniform_actions"] == [4, 2] and out["types"][0]["avg_reward"] == want["types"][0]["avg_reward"]
    assert out["types"][1]["avg_reward"] == want["types"][1]["avg_reward"]


def test_graph_capture():
    """rollout_eval_drawn captured with static keys, draw keys, state, stats and actions_out (E = 5,
    T = 8): two replays from the same inputs give the bits of each other and of the eager call"""
    cfg = builtin_config(FQ)
    E, T = 5, 8
    env = MARLEnv(None, cfg, data=_day(cfg.world_config, 2_000_000), persistent_outputs=True)
    params = env.default_params
    k0 = torch.from_numpy(np.arange(2 * E, dtype=np.uint32).reshape(E, 2).view(np.int32) + 3).cuda()
    _, state = env.reset(k0, params)
    start = state.buf.clone()
    keys = split_keys(k0, T).transpose(0, 1).contiguous()
    dk = _dev_key(draw_keys_numpy(17, T, 2))
    masks = [Uniform.all().mask(sp.n) for sp in env.action_spaces]
    gst = torch.zeros((E, env.num_agents, 106), dtype=torch.float64, device="cuda")
    acts = torch.zeros((T, E, env.action_words), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # the eager call, outside the capture
        env.rollout_eval_drawn(keys, state, dk, masks, params, stats=gst, actions_out=acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = (state.buf.clone(), gst.clone(), acts.clone())
    assert not torch.equal(eager[0], start)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.rollout_eval_drawn(keys, state, dk, masks, params, stats=gst, actions_out=acts)
    for tag in ("first", "second"):
        state.buf.copy_(start)
        gst.zero_()
        acts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(state.buf, eager[0]), f"{tag} replay: end state"
        assert torch.equal(gst, eager[1]), f"{tag} replay: stats"
        assert torch.equal(acts, eager[2]), f"{tag} replay: actions_out"
