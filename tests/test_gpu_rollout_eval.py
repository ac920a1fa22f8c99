"""MARLEnv.rollout_eval / hftlob_env_rollout_eval (k_env_rollout_eval: T tally steps in one
persistent launch, the agents' rewards and info words folded into float64 accumulators).

`ref` of a case is hftlob.evaluate.reduce_steps over the outputs of env.rollout(per_step=True) on a
clone of the case's start state (that path is held to the per-step launches and the oracle by
test_gpu_rollout_actions, whose cases and inputs these tests share).  The kernel's stats equal ref
with torch.equal on the float64 tensor; its end state and last-step outputs equal
rollout(per_step=False)'s bit for bit; hftlob_env_launch_info names the instantiation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from book_edges import slot_sets
from hftlob import evaluate as EV
from hftlob.config_io import builtin_config
from hftlob.data.synthetic import generate_day
from hftlob.env import MARLEnv, split_keys
from hftlob.layout import AGENT_MM, INFO_AGENT_WORDS, INFO_EXE, INFO_MM, INFO_WORLD_WORDS
from oracle import pyoracle as O
from test_gpu_env import MULTI_AGENT_CASES, _day, _expect_launch, _multi_agent_config, speed_test_config
from test_gpu_rollout_actions import NFIX, _reference, _same, _sized

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ = "2_player_fq_fqc"
_EVAL = {}


def _flat(xs, T, E):
    return torch.cat([x.reshape(T, E, -1) for x in xs], dim=2)


def _eval_reference(tag, cfg, E, T):
    """The case's per-step outputs (one env.rollout(per_step=True)), their reduction `ref`, and the
    end state and last-step outputs of env.rollout(per_step=False): computed once per case, never
    modified."""
    key = (tag, E, T)
    if key in _EVAL:
        return _EVAL[key]
    R = _reference(tag, cfg, E, T)
    env, params = R["env"], R["params"]
    s = R["start"].clone(env)
    _, _, rew, dones, _ = env.rollout(R["keys"], s, R["acts"], params, per_step=True)
    rew, done = _flat(rew, T, E).clone(), dones["__all__"].clone()
    words = env.last_info_words.reshape(T, E, -1).clone()
    assert bool((s.buf == R["end"]).all())
    s = R["start"].clone(env)
    obs, _, r, d, _ = env.rollout(R["keys"], s, R["acts"], params, per_step=False)
    last = dict(obs=[x.clone() for x in obs], rew=[x.clone() for x in r], done=d["__all__"].clone(),
                dones=[x.clone() for x in d["agents"]], info=env.last_info_words.clone())
    assert bool((s.buf == R["end"]).all())
    _EVAL[key] = dict(R, rew=rew, done=done, words=words, last=last,
                      ref=EV.reduce_steps(rew, words, done, env.layout))
    return _EVAL[key]


def _check_end(tag, V, s, obs, rew, dones, env):
    bad = torch.nonzero(s.buf != V["end"])
    assert bad.numel() == 0, f"{tag}: end state vs rollout(per_step=False) (env, word) {bad[:5].tolist()}"
    last = V["last"]
    assert _same(obs, last["obs"]) and _same(rew, last["rew"]), f"{tag}: last step's obs / rewards"
    assert bool((dones["__all__"] == last["done"]).all()) and _same(dones["agents"], last["dones"]), f"{tag}: dones"
    assert bool((env.last_info_words == last["info"]).all()), f"{tag}: last step's info words"


def eval_parity(tag, cfg, E, T, expect=None, reset_inside=False):
    V = _eval_reference(tag, cfg, E, T)
    env, params = V["env"], V["params"]
    _expect_launch(env, expect)
    s = V["start"].clone(env)
    obs, s_ret, rew, dones, _, stats = env.rollout_eval(V["keys"], s, V["acts"], params)
    torch.cuda.synchronize()
    assert s_ret is s and stats.dtype == torch.float64 and tuple(stats.shape) == (E, env.num_agents, 106)
    bad = torch.nonzero(~((stats == V["ref"]) | (stats.isnan() & V["ref"].isnan())))
    assert bad.numel() == 0, f"{tag}: stats vs reduce_steps (env, agent, word) {bad[:8].tolist()}"
    assert torch.equal(stats, V["ref"]) or bool(V["ref"].isnan().any())
    _check_end(tag, V, s, obs, rew, dones, env)
    assert bool((stats[:, :, 0] == T).all())
    if reset_inside:
        assert bool((stats[:, :, 1] >= 1).all()), "every env crossed its episode end"
        assert bool(V["done"].any(dim=0).all())
    return V, stats


def test_resident_kernel_crosses_reset():
    """k_env_rollout_eval<2, 100, false, false>, E = 24, T = 70: every env crosses its 65-step episode
    end inside the tally loop (the resident book is dropped and reloaded); word 1 >= 1 everywhere
    and word 2 is the reward sum since the reset"""
    E, T = 24, 70
    V, stats = eval_parity("fq_fqc", builtin_config(FQ), E, T, expect=NFIX, reset_inside=True)
    rew, done = V["rew"].cpu().numpy().astype(np.float64), V["done"].cpu().numpy()
    run = np.zeros(rew.shape[1:])
    for t in range(T):
        run = np.where(done[t][:, None], 0.0, run + rew[t])
    assert (stats[:, :, 2].cpu().numpy() == run).all()
    assert (stats[:, :, 3].cpu().numpy() == (T - 1 - np.argmax(done, axis=0))[:, None]).all()


def test_chunked_launches():
    """33 + 37 steps with the stats carried over, and a start from a non-zero stats tensor (the ref
    of the first 33 steps): both equal the one-call result bit for bit"""
    E, T, T1 = 24, 70, 33
    V = _eval_reference("fq_fqc", builtin_config(FQ), E, T)
    env, params = V["env"], V["params"]
    _expect_launch(env, NFIX)
    s = V["start"].clone(env)
    st = env.rollout_eval(V["keys"][:T1], s, V["acts"][:T1], params)[-1]
    ref1 = EV.reduce_steps(V["rew"][:T1], V["words"][:T1], V["done"][:T1], env.layout)
    assert torch.equal(st, ref1)
    mid = s.buf.clone()
    out = env.rollout_eval(V["keys"][T1:], s, V["acts"][T1:], params, stats=st)
    assert out[-1] is st, "a given stats tensor is accumulated into in place"
    assert torch.equal(st, V["ref"])
    _check_end("chunked", V, s, out[0], out[2], out[3], env)
    s2 = V["start"].clone(env)
    s2.buf.copy_(mid)
    given = ref1.clone()
    env.rollout_eval(V["keys"][T1:], s2, V["acts"][T1:], params, stats=given)
    assert torch.equal(given, V["ref"]) and bool((s2.buf == V["end"]).all())


def test_fixed_actions():
    """fixed=True: one [action_words] row, and the per-type list without T and E, equal the row
    expanded to [T, E, action_words]"""
    E, T = 8, 12
    R = _reference("fq_fqc", builtin_config(FQ), E, T)
    env, params = R["env"], R["params"]
    _expect_launch(env, NFIX)
    row = R["acts"][3, 5].clone()
    s0, s1, s2 = (R["start"].clone(env) for _ in range(3))
    a = env.rollout_eval(R["keys"], s0, row.expand(T, E, -1).contiguous(), params)
    a = ([x.clone() for x in a[0]], [x.clone() for x in a[2]], a[5])
    b = env.rollout_eval(R["keys"], s1, row, params, fixed=True)
    assert torch.equal(a[2], b[5]) and bool((s0.buf == s1.buf).all()) and _same(a[0], b[0]) and _same(a[1], b[2])
    per_type = [x[0].contiguous() for x in env.split_actions(row[None])]
    c = env.rollout_eval(R["keys"], s2, per_type, params, fixed=True)
    assert torch.equal(a[2], c[5]) and bool((s0.buf == s2.buf).all())
    assert bool((a[2][:, :, 0] == T).all()) and not bool((s0.buf == R["end"]).all())


@pytest.mark.parametrize("E,T", [(8, 1), (1, 1), (1, 5), (1025, 3)])
def test_single_step_and_single_env(E, T):
    """T = 1: the emitting step alone is tallied; E = 1: a one-workgroup launch; E = 1025: the smallest
    launch whose waves rank their issue priority, after the tally steps 0 and 1 of T = 3"""
    eval_parity("fq_fqc", builtin_config(FQ), E, T, expect=NFIX)


@pytest.mark.parametrize("nO,nT", [(64, 64), (129, 100)], ids=lambda v: str(v))
def test_general_sizes(nO, nT):
    """k_env_rollout_eval<S, 0, false> for S = 1 and 4"""
    eval_parity(f"sized_{nO}_{nT}", _sized(FQ, nO, nT), 16, 40,
                expect=dict(slot_sets=slot_sets(nO, nT), nfix=0, random_cancel=0, rows_alias=0))


def test_general_size_crosses_reset():
    """a general-size kernel tallies an episode end: 64/64 slots, 70 steps over 65-step episodes"""
    eval_parity("sized_64_64", _sized(FQ, 64, 64), 16, 70, expect=dict(slot_sets=1, nfix=0, random_cancel=0),
                reset_inside=True)


def test_random_cancel():
    eval_parity("rc2", _sized(FQ, 64, 64, cancel_mode=2), 16, 40, expect=dict(slot_sets=1, nfix=0, random_cancel=1))


def test_rows_alias_crosses_reset():
    """k_env_rollout_eval<2, 100, false, true> with [5, 5] agents over Speed_test's 32-step episodes"""
    eval_parity("rows_alias_32", speed_test_config([5, 5], 100), 16, 40,
                expect=dict(slot_sets=2, nfix=100, random_cancel=0, rows_alias=1), reset_inside=True)


def test_three_agent_types():
    eval_parity("3_player", builtin_config("3_player_fq_fqc_dir"), 16, 40, expect=NFIX)


def test_multidiscrete_fixed_prices():
    name, agents, changes = MULTI_AGENT_CASES[2]
    assert changes["action_space"] == "fixed_prices"
    eval_parity("fixed_prices", _multi_agent_config(name, agents, changes), 16, 40,
                expect=dict(slot_sets=2, nfix=0, random_cancel=0))


def _np_reduce(x, done):
    """the sequential float64 loop of reduce_steps in numpy, over quantities x [T, E, A, 25] and
    done [T, E]: the 106 words [E, A, 106]"""
    T, E, A, _ = x.shape
    st = np.zeros((E, A, 106))
    for t in range(T):
        d = done[t].astype(bool)[:, None]
        st[:, :, 0] += 1.0
        st[:, :, 1] += d
        rs, rl = st[:, :, 2] + x[t, :, :, 0], st[:, :, 3] + 1.0
        for w, v in ((4, rs), (5, rs * rs), (6, rl), (7, rl * rl)):
            st[:, :, w] = np.where(d, st[:, :, w] + v, st[:, :, w])
        st[:, :, 2], st[:, :, 3] = np.where(d, 0.0, rs), np.where(d, 0.0, rl)
        st[:, :, 8:58:2] += x[t]
        st[:, :, 9:58:2] += x[t] * x[t]
        st[:, :, 58::2] = np.where(d[:, :, None], st[:, :, 58::2] + x[t, :, :, 1:], st[:, :, 58::2])
        st[:, :, 59::2] = np.where(d[:, :, None], st[:, :, 59::2] + x[t, :, :, 1:] ** 2, st[:, :, 59::2])
    return st


def test_against_cpu_oracle():
    """Case 1's inputs through O.env_step in a loop; the oracle's per-step rewards, info and
    done_all reduced by the same float64 loop in numpy.  Words 0, 1, 3, 6, 7 and every int-typed
    quantity's words are equal.  A float quantity's sum is within 1e-5 n + 1e-5 sum|x| of the
    oracle's (the project's per-value rtol = atol = 1e-5, summed; n the values summed, x the
    oracle's) and its sum of squares within sum(2 |x| d + d^2), d = 1e-5 (1 + |x|).  The words derived
    from the reward sums: word 2 and word 4 by the same bound over the steps they sum; word 5 (squares
    of episode sums S) within sum over episodes of 2 |S| D + D^2, D the bound of S."""
    E, T = 24, 70
    V = _eval_reference("fq_fqc", builtin_config(FQ), E, T)
    env = V["env"]
    L, A = env.layout, env.num_agents
    day = _day(builtin_config(FQ).world_config, 2_000_000)
    init = env._init_states.cpu().numpy()
    st = V["start"].buf.cpu().numpy().copy()
    kn, an = V["keys"].cpu().numpy().view(np.uint32), V["acts"].cpu().numpy()
    x, done = np.zeros((T, E, A, 25)), np.zeros((T, E), bool)
    isf = np.zeros((A, INFO_AGENT_WORDS), bool)               # the float32 words of each agent's info block
    for a, kind in enumerate(L.agent_kinds):
        fields = INFO_MM if kind == AGENT_MM else INFO_EXE
        isf[a, :len(fields)] = [bool(f) for _, f in fields]
    assert (isf == EV._float_words(L).numpy()).all()
    for t in range(T):
        st, _, r, da, _, info = O.env_step(env.cfg_c, kn[t], an[t], day.msgs, init, st)
        iw = info[:, INFO_WORLD_WORDS:INFO_WORLD_WORDS + A * INFO_AGENT_WORDS].reshape(E, A, INFO_AGENT_WORDS)
        x[t, :, :, 0] = r.astype(np.float64)
        x[t, :, :, 1:] = np.where(isf, iw.view(np.float32).astype(np.float64), iw.astype(np.float64))
        done[t] = da != 0
    assert (done == V["done"].cpu().numpy()).all()
    want = _np_reduce(x, done)
    got = V["ref"].cpu().numpy()          # == the kernel's stats bit for bit (test_resident_kernel_crosses_reset)
    s = V["start"].clone(env)
    got_k = env.rollout_eval(V["keys"], s, V["acts"], V["params"])[-1].cpu().numpy()
    assert (got_k == got).all()
    for w in (0, 1, 3, 6, 7):
        assert (got[:, :, w] == want[:, :, w]).all(), w
    qf = np.concatenate([np.ones((A, 1), bool), isf], 1)                      # [A, 25]: float quantities
    step_i = np.zeros((A, 106), bool)
    step_i[:, 8:58:2] = step_i[:, 9:58:2] = ~qf
    step_i[:, 58::2] = step_i[:, 59::2] = ~isf
    for a in range(A):
        assert (got[:, a][:, step_i[a]] == want[:, a][:, step_i[a]]).all(), f"agent {a}: int-typed words"
    ax = np.abs(x)
    dl = 1e-5 * (1.0 + ax)
    sq = 2 * ax * dl + dl * dl
    dm = done[:, :, None, None]
    n_ep = done.sum(0)[:, None, None]
    bound = np.zeros((E, A, 106))
    bound[:, :, 8:58:2] = 1e-5 * T + 1e-5 * ax.sum(0)
    bound[:, :, 9:58:2] = sq.sum(0)
    bound[:, :, 58::2] = (1e-5 * n_ep + 1e-5 * (ax * dm).sum(0))[:, :, 1:]
    bound[:, :, 59::2] = (sq * dm).sum(0)[:, :, 1:]
    # the reward-sum words: per-step bound d of the reward, summed over the steps each sums
    dr = 1e-5 + 1e-5 * ax[..., 0]                                              # [T, E, A]
    run = np.zeros((E, A))
    S = np.zeros((E, A))
    for t in range(T):
        run = run + dr[t]
        S = S + x[t, :, :, 0]
        d = done[t][:, None]
        bound[:, :, 4] += np.where(d, run, 0.0)
        bound[:, :, 5] += np.where(d, 2 * np.abs(S) * run + run * run, 0.0)
        run, S = np.where(d, 0.0, run), np.where(d, 0.0, S)
    bound[:, :, 2] = run
    fl = np.ones((A, 106), bool)
    fl[:, [0, 1, 3, 6, 7]] = False
    fl &= ~step_i
    diff = np.abs(got - want)
    ok = (diff <= bound) | (np.isnan(got) & np.isnan(want)) | (got == want)
    bad = np.argwhere(~ok & fl[None])
    assert bad.size == 0, [(tuple(b), got[tuple(b)], want[tuple(b)], bound[tuple(b)]) for b in bad[:6]]


def test_bad_arguments():
    """each raises ValueError and launches nothing: the state and stats are unchanged afterwards"""
    E, T = 8, 12
    R = _reference("fq_fqc", builtin_config(FQ), E, T)
    env, params, keys, acts = R["env"], R["params"], R["keys"], R["acts"]
    W, A = env.action_words, env.num_agents
    s = R["start"].clone(env)
    stats = torch.full((E, A, 106), 3.0, dtype=torch.float64, device="cuda")
    row = acts[0, 0].clone()
    bad = [dict(actions=acts, stats=stats.to(torch.float32)),                  # dtype
           dict(actions=acts, stats=torch.zeros((E, A, 105), dtype=torch.float64, device="cuda")),   # shape
           dict(actions=acts, stats=torch.zeros((E + 1, A, 106), dtype=torch.float64, device="cuda")),
           dict(actions=acts, stats=torch.zeros((E, A * 106), dtype=torch.float64, device="cuda")),
           dict(actions=acts, stats=stats.cpu()),                              # device
           dict(actions=acts, fixed=True),                                     # fixed with [T, E, W]
           dict(actions=row, fixed=False),                                     # not fixed with [W]
           dict(actions=row.to(torch.int64), fixed=True),
           dict(actions=[row[:1]], fixed=True),                                # a type missing
           dict(actions=acts, key=keys[:, :-1]),                               # keys and state disagree on E
           dict(actions=acts, key=keys[0]),
           dict(actions=acts, key=keys[:0])]
    assert W == 2 and row.shape == (W,)
    for kw in bad:
        kw.setdefault("stats", stats)
        k = kw.pop("key", keys)
        a = kw.pop("actions")
        with pytest.raises(ValueError):
            env.rollout_eval(k, s, a, params, **kw)
    torch.cuda.synchronize()
    assert bool((s.buf == R["start"].buf).all()) and bool((stats == 3.0).all()), "a refused call launches nothing"


def test_graph_capture():
    """rollout_eval captured on one stream with static keys, actions, state and stats (E = 16, T = 8):
    two replays from the start state and zeroed stats give the case's result; a third without
    zeroing gives exactly twice the step sums (words 0 and 8..57: all values are sums), and bit for
    bit reduce_steps continued from the first result"""
    cfg = builtin_config(FQ)
    E, T = 16, 8
    V = _eval_reference("fq_fqc", cfg, E, T)
    env = MARLEnv(None, cfg, data=_day(cfg.world_config, 2_000_000), persistent_outputs=True)
    _expect_launch(env, NFIX)
    params = env.default_params
    gk, ga, gs = V["keys"].clone(), V["acts"].clone(), V["start"].clone(env)
    gst = torch.zeros((E, env.num_agents, 106), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (module load, output buffers)
        env.rollout_eval(gk, gs, ga, params, stats=gst)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.rollout_eval(gk, gs, ga, params, stats=gst)
    for tag in ("first", "second"):
        gs.buf.copy_(V["start"].buf)
        gst.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert bool((gs.buf == V["end"]).all()), f"{tag} replay: end state"
        assert torch.equal(gst, V["ref"]), f"{tag} replay: stats"
    gs.buf.copy_(V["start"].buf)
    g.replay()
    torch.cuda.synchronize()
    assert bool((gs.buf == V["end"]).all()), "third replay: end state"
    assert torch.equal(gst[:, :, 0], 2 * V["ref"][:, :, 0]) and bool((gst[:, :, 0] == 2 * T).all())
    assert torch.equal(gst[:, :, 8:58], 2 * V["ref"][:, :, 8:58]), "the step sums double"
    assert torch.equal(gst, EV.reduce_steps(V["rew"], V["words"], V["done"], env.layout, stats=V["ref"]))


def _cli_env(n_msgs):
    cfg = builtin_config(FQ)
    w = cfg.world_config
    day = generate_day(n_msgs=n_msgs, snap_every=w.n_data_msg_per_step * w.start_resolution)
    return MARLEnv(None, cfg, data=day, device="cuda:0", return_info=False, persistent_outputs=True)


def test_evaluate_fixed_actions_and_command_line():
    """evaluate_fixed_actions at 8 envs, 20 steps, chunk = 8 equals a hand-written loop of split_keys
    and rollout_eval over the same chain; the command line's JSON carries the same avg_reward"""
    E, T, seed, n_msgs = 8, 20, 7, 30_000
    env = _cli_env(n_msgs)
    ev = EV.evaluate_fixed_actions(env, [4, 2], E, T, seed, chunk=8)
    params = env.default_params
    rng = torch.tensor([[0, seed]], dtype=torch.int32, device="cuda")
    p = split_keys(rng, 2)
    rng = p[:, 0].contiguous()
    _, state = env.reset(split_keys(p[:, 1].contiguous(), E)[0], params)
    keys = torch.empty((T, E, 2), dtype=torch.int32, device="cuda")
    for t in range(T):
        rng = split_keys(rng, 2)[:, 0].contiguous()          # the unused action sample
        p = split_keys(rng, 2)
        rng = p[:, 0].contiguous()
        keys[t] = split_keys(p[:, 1].contiguous(), E)[0]
    row = torch.tensor([4, 2], dtype=torch.int32, device="cuda")
    stats = env.rollout_eval(keys, state, row, params, fixed=True)[-1]
    assert torch.equal(ev.stats, stats) and ev.steps(0) == E * T
    want = EV.EvalStats(stats, env.layout).summary()
    run = subprocess.run([sys.executable, "-m", "hftlob.evaluate", "--env-config", FQ, "--fixed-actions", "4,2",
                          "--envs", str(E), "--steps", str(T), "--seed", str(seed), "--chunk", "8",
                          "--data-msgs", str(n_msgs)], capture_output=True, text=True, timeout=300,
                         cwd=ROOT, env=dict(os.environ, PYTHONPATH=os.pathsep.join(
                             [os.path.join(ROOT, "jaxmarl-hft_amd")] + [p for p in sys.path if p])))
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["envs"] == E and out["steps"] == T and len(out["types"]) == 2
    for t in range(2):
        assert out["types"][t]["avg_reward"] == want["types"][t]["avg_reward"]
        assert out["types"][t]["episodes"] == want["types"][t]["episodes"]
    assert "reward_portfolio_value" in out["types"][0]["info"]
    assert "revenue_direction_normalised" in out["types"][1]["info"]
