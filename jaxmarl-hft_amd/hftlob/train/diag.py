"""Per-update training diagnostics tallied on the device (the ``TRAIN_DIAG`` switch of ``train.ippo``): what
the reference's update callback (ippo_rnn_JAXMARL.py:977-1059) logs from the trajectory batch, without a
trajectory of info dicts.

* :func:`rollout_diag` reduces one agent type's rollout buffers (actions, reward, value, log-prob, advantage,
  target, global done) to ``DIAG_WORDS`` doubles as two HIP launches (hftlob_rollout_diag; include/hftlob.h has
  the word table and the order of every sum); :func:`rollout_diag_reference` is its definition in torch float64,
  in that order, bit for bit, and the path on a CPU device.
* :func:`world_tally` folds the world info words of per-step info records into per-env sums
  (hftlob_world_tally), the world half of ``evaluate.tally_steps``; :func:`world_tally_reference` is its
  definition.
* :class:`RolloutTally` holds the fixed-address accumulators of a rollout and is what ``rollout_members`` calls
  per step (one agents' tally and one world tally for the whole env batch, capturable in a HIP graph).
* :class:`TrainDiag` is ``metrics["diag"]``: clones of an update's accumulators, read only when asked.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import torch

from .. import _lib
from .._lib import (DIAG_MAX_ACTIONS, DIAG_MAX_HEADS, DIAG_MAX_STRIPES, DIAG_STRIPE_ROWS, DIAG_WORDS, EVAL_WORDS,
                    WORLD_TALLY_WORDS)
from ..layout import INFO_WORLD, INFO_WORLD_WORDS

# words of hftlob_rollout_diag's result (include/hftlob.h)
D_N, D_DONES = 0, 1
D_Q = 2                 # + 2q, + 2q + 1: the sum and sum of squares of quantity q
QUANTITIES = ("reward", "value", "log_prob", "advantage", "target", "residual")
D_ACT_SUM = 14          # + k: the sum of head k's in-range action words
D_ACT_OOR = 18          # + k: head k's words outside [0, nvec[k])
D_ACT_BIN = 22          # + 16k + a: the count of head k's action a
LANES = 256             # the lanes of the partial pass's workgroup: lane l adds elements l, l + 256, ...
assert D_Q + 2 * len(QUANTITIES) == D_ACT_SUM and D_ACT_BIN + DIAG_MAX_HEADS * DIAG_MAX_ACTIONS == DIAG_WORDS
assert WORLD_TALLY_WORDS == 2 * INFO_WORLD_WORDS == 2 * len(INFO_WORLD)
WORLD_FLOAT_WORDS = sum(1 << k for k, (_, isf) in enumerate(INFO_WORLD) if isf)


def stripe_rows(N: int) -> int:
    """the elements of a stripe of hftlob_rollout_diag's partial pass (the header's rule, from N alone)"""
    return DIAG_STRIPE_ROWS if -(-N // DIAG_STRIPE_ROWS) <= DIAG_MAX_STRIPES else -(-N // DIAG_MAX_STRIPES)


def stripes(N: int) -> int:
    """the number of stripes (none is empty); 0 for N = 0"""
    return -(-N // stripe_rows(N)) if N > 0 else 0


def diag_workspace(N: int) -> int:
    """hftlob_rollout_diag_workspace(N) restated: the doubles of the caller's workspace"""
    return stripes(N) * DIAG_WORDS


def _check_heads(nvec) -> List[int]:
    nvec = [int(n) for n in ([nvec] if isinstance(nvec, int) else nvec)]
    if not 1 <= len(nvec) <= DIAG_MAX_HEADS or any(not 1 <= n <= DIAG_MAX_ACTIONS for n in nvec):
        raise ValueError(f"rollout_diag takes 1..{DIAG_MAX_HEADS} heads of 1..{DIAG_MAX_ACTIONS} actions, got {nvec}")
    return nvec


def diag_supported(heads: Sequence[int]) -> bool:
    """whether a net with these head widths is within hftlob_rollout_diag's limits"""
    return 1 <= len(heads) <= DIAG_MAX_HEADS and all(1 <= int(n) <= DIAG_MAX_ACTIONS for n in heads)


def _diag_inputs(buf, adv, target, nvec):
    """(action [N, K] int32, the five float32 [N] arrays in word order, done [N] uint8, nvec) of a ``Rollout``
    (its ``global_done`` is the done) or of the sequence (action, reward, value, log_prob, done), checked."""
    nvec = _check_heads(nvec)
    if hasattr(buf, "global_done"):
        action, reward, value, log_prob, done = buf.action, buf.reward, buf.value, buf.log_prob, buf.global_done
    else:
        action, reward, value, log_prob, done = buf
    fl = (reward, value, log_prob, adv, target)
    for name, x in zip(("action", "reward", "value", "log_prob", "adv", "target", "done"), (action,) + fl + (done,)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"rollout_diag: {name} must be a tensor")
    dev, N = reward.device, reward.numel()
    if action.dtype != torch.int32 or action.numel() != N * len(nvec):
        raise ValueError(f"rollout_diag: action must be int32 with {len(nvec)} words per element ({N} elements)")
    for name, x in zip(("reward", "value", "log_prob", "adv", "target"), fl):
        if x.dtype != torch.float32 or x.numel() != N:
            raise ValueError(f"rollout_diag: {name} must be float32 with {N} elements")
    if done.dtype not in (torch.bool, torch.uint8) or done.numel() != N:
        raise ValueError(f"rollout_diag: done must be bool or uint8 with {N} elements")
    for name, x in zip(("action", "reward", "value", "log_prob", "adv", "target", "done"), (action,) + fl + (done,)):
        if x.device != dev:
            raise ValueError(f"rollout_diag: {name} is on {x.device}, reward on {dev}")
        if not x.is_contiguous():
            raise ValueError(f"rollout_diag: {name} must be contiguous")
    if done.dtype == torch.bool:
        done = done.view(torch.uint8)
    return action.view(N, len(nvec)), [x.view(N) for x in fl], done.view(N), nvec


def rollout_diag(buf, adv: torch.Tensor, target: torch.Tensor, nvec, out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hftlob_rollout_diag (csrc/rollout_diag.hip) on torch's current stream: the ``DIAG_WORDS`` float64 words of
    one agent type's rollout, bit for bit :func:`rollout_diag_reference`.
    buf: a ``train.ippo.Rollout`` (its action, reward, value, log_prob and global_done are read), or the
    sequence (action, reward, value, log_prob, done); adv, target: the update's advantages and targets; nvec:
    the heads' widths (an int for one head).  action is int32 with len(nvec) words per element, the five
    others float32, done bool or uint8; all contiguous, on one GPU device, with the same number N of elements
    (any shape).  out: a contiguous float64 [DIAG_WORDS] tensor on that device to write (None allocates one);
    workspace: a contiguous float64 tensor of at least ``diag_workspace(N)`` elements (None allocates one).
    With both given the call allocates nothing, does not synchronise and can be captured in a HIP graph."""
    action, fl, done, nvec = _diag_inputs(buf, adv, target, nvec)
    dev, N = fl[0].device, fl[0].numel()
    if dev.type != "cuda":
        raise ValueError(f"rollout_diag needs its tensors on a GPU device, got {dev} (rollout_diag_reference is the "
                         "CPU path)")
    need = diag_workspace(N)
    if out is None:
        out = torch.empty(DIAG_WORDS, dtype=torch.float64, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (DIAG_WORDS,)
          or out.device != dev or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float64 [{DIAG_WORDS}] tensor on {dev}")
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float64 or workspace.numel() < need
          or workspace.device != dev or not workspace.is_contiguous()):
        raise ValueError(f"workspace must be a contiguous float64 tensor of >= {need} elements on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hftlob_rollout_diag(N, len(nvec), (C.c_int * len(nvec))(*nvec), _lib.ptr(action),
                                                  *[_lib.ptr(x) for x in fl], _lib.ptr(done), _lib.ptr(out),
                                                  _lib.ptr(workspace), _lib.stream_ptr(device=dev)))
    return out


def rollout_diag_reference(buf, adv: torch.Tensor, target: torch.Tensor, nvec) -> torch.Tensor:
    """The definition of hftlob_rollout_diag: :func:`rollout_diag`'s arguments (on any device), its float64
    [DIAG_WORDS] result on the inputs' device, in the header's order of every sum.  The elements are cut into
    ``stripes(N)`` stripes of ``stripe_rows(N)``; in a stripe lane l of 256 adds the elements l, l + 256, ... in
    that order from +0.0, the stripe's partial is the lanes' sums added in lane order, and the result is the
    stripes' partials added in stripe order.  Counts are integers."""
    action, fl, done, nvec = _diag_inputs(buf, adv, target, nvec)
    dev, N = fl[0].device, fl[0].numel()
    out = torch.zeros(DIAG_WORDS, dtype=torch.float64, device=dev)
    if N == 0:
        return out
    x = torch.stack([v.to(torch.float64) for v in fl] + [fl[4].to(torch.float64) - fl[1].to(torch.float64)])
    xs = torch.stack([x, x * x], dim=1).reshape(2 * len(QUANTITIES), N)      # rows 2q, 2q + 1: words 2 + 2q, 3 + 2q
    rows, G = stripe_rows(N), stripes(N)
    per = -(-rows // LANES)                                                   # a lane's elements in a full stripe
    # [word, stripe, lane's j-th element, lane], +0.0 where the stripe or the rollout has no element
    pad = torch.zeros((xs.shape[0], G * rows), dtype=torch.float64, device=dev)
    pad[:, :N] = xs
    cell = torch.zeros((xs.shape[0], G, per * LANES), dtype=torch.float64, device=dev)
    cell[:, :, :rows] = pad.view(xs.shape[0], G, rows)
    cell = cell.view(xs.shape[0], G, per, LANES)
    lane = torch.zeros((xs.shape[0], G, LANES), dtype=torch.float64, device=dev)
    for j in range(per):
        lane = lane + cell[:, :, j]
    part = lane[:, :, 0].clone()
    for l in range(1, LANES):
        part = part + lane[:, :, l]
    tot = part[:, 0].clone()
    for g in range(1, G):
        tot = tot + part[:, g]
    out[D_Q:D_ACT_SUM] = tot
    out[D_N] = float(N)
    out[D_DONES] = float(int((done != 0).sum().item()))
    a64 = action.to(torch.int64)
    for k, n in enumerate(nvec):
        ok = (a64[:, k] >= 0) & (a64[:, k] < n)
        bins = torch.bincount(a64[:, k][ok], minlength=DIAG_MAX_ACTIONS)
        out[D_ACT_BIN + DIAG_MAX_ACTIONS * k:D_ACT_BIN + DIAG_MAX_ACTIONS * (k + 1)] = bins.to(torch.float64)
        out[D_ACT_SUM + k] = float(int(a64[:, k][ok].sum().item()))
        out[D_ACT_OOR + k] = float(int((~ok).sum().item()))
    return out


def _check_info(info_words: torch.Tensor) -> torch.Tensor:
    if not isinstance(info_words, torch.Tensor) or info_words.dtype != torch.int32 or info_words.dim() != 3 \
            or info_words.shape[2] < INFO_WORLD_WORDS or info_words.shape[0] < 1 or info_words.shape[1] < 1:
        raise ValueError(f"info_words must be int32 [T >= 1, E >= 1, info_words >= {INFO_WORLD_WORDS}]")
    return info_words


def _check_wstats(wstats, E: int, dev, contiguous: bool) -> None:
    if (not isinstance(wstats, torch.Tensor) or wstats.dtype != torch.float64
            or tuple(wstats.shape) != (E, WORLD_TALLY_WORDS) or wstats.device != dev
            or (contiguous and not wstats.is_contiguous())):
        raise ValueError(f"wstats must be a{' contiguous' if contiguous else ''} float64 [{E}, {WORLD_TALLY_WORDS}] "
                         f"tensor on {dev}")


def _world_launch(info_words: torch.Tensor, wstats: torch.Tensor) -> None:
    """hftlob_world_tally on checked device tensors ([T, E, info_w] int32, [E, WORLD_TALLY_WORDS]), adding to wstats"""
    T, E, info_w = info_words.shape
    dev = info_words.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hftlob_world_tally(E, T, info_w, _lib.ptr(info_words), WORLD_FLOAT_WORDS,
                                                 _lib.ptr(wstats), _lib.stream_ptr(device=dev)))


def world_tally(info_words: torch.Tensor, wstats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`world_tally_reference` as one launch of hftlob_world_tally on torch's current stream: the same bits.
    info_words: the raw info records, contiguous int32 [T, E, info_words] on a GPU.  Unlike the reference a given
    ``wstats`` (contiguous float64 [E, WORLD_TALLY_WORDS] on that device) is continued IN PLACE; None starts from
    zeros.  Returns the wstats tensor."""
    info_words = _check_info(info_words)
    dev, E = info_words.device, info_words.shape[1]
    if dev.type != "cuda" or not info_words.is_contiguous():
        raise ValueError(f"world_tally needs a contiguous info_words on a GPU device, got {dev}")
    if wstats is None:
        wstats = torch.zeros((E, WORLD_TALLY_WORDS), dtype=torch.float64, device=dev)
    else:
        _check_wstats(wstats, E, dev, True)
    _world_launch(info_words, wstats)
    return wstats


def world_tally_reference(info_words: torch.Tensor, wstats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition of hftlob_world_tally: a sequential float64 loop over the steps, on the input's device.
    Word 2k of an env's row is the sum of world info word k over the steps in step order (widened from int32,
    or from the float32 with the same bits where ``layout.INFO_WORLD`` says so), word 2k + 1 the sum of its
    squares.  wstats: float64 [E, WORLD_TALLY_WORDS] to continue from (not modified); None starts from zeros.
    Returns the new tensor."""
    info_words = _check_info(info_words)
    dev, (T, E) = info_words.device, info_words.shape[:2]
    if wstats is None:
        st = torch.zeros((E, WORLD_TALLY_WORDS), dtype=torch.float64, device=dev)
    else:
        _check_wstats(wstats, E, dev, False)
        st = wstats.clone()
    w = info_words[:, :, :INFO_WORLD_WORDS].contiguous()
    isf = torch.tensor([bool(f) for _, f in INFO_WORLD], device=dev)
    x = torch.where(isf, w.view(torch.float32).to(torch.float64), w.to(torch.float64))
    x2 = x * x
    for t in range(T):
        st[:, 0::2] += x[t]
        st[:, 1::2] += x2[t]
    return st


class RolloutTally:
    """The accumulators of a rollout's per-step tallies for one env batch of ``E`` envs, allocated once (fixed
    addresses: a captured rollout replays into them): ``stats`` float64 [E, n_agents, EVAL_WORDS]
    (``evaluate.reduce_steps``' words) and ``wstats`` float64 [E, WORLD_TALLY_WORDS].  On a GPU a step is one
    hftlob_eval_tally and one hftlob_world_tally launch on the current stream; on the CPU the reference
    functions."""

    def __init__(self, env, E: int, device):
        from ..evaluate import _float_word_masks
        self.layout = env.layout
        self.device = torch.device(device)
        A = len(self.layout.agent_kinds)
        self.stats = torch.zeros((E, A, EVAL_WORDS), dtype=torch.float64, device=self.device)
        self.wstats = torch.zeros((E, WORLD_TALLY_WORDS), dtype=torch.float64, device=self.device)
        self._masks = _float_word_masks(self.layout)

    def begin(self) -> None:
        """The top of a rollout: every word to zero but the running episode's reward sum and length (words 2
        and 3), which carry across updates so that an episode spanning two rollouts counts whole."""
        self.stats[:, :, :2].zero_()
        self.stats[:, :, 4:].zero_()
        self.wstats.zero_()

    def step(self, env, dones) -> None:
        """One env step's tally from ``env.last_rewards``, ``env.last_info_words`` and ``dones["__all__"]``."""
        from ..evaluate import _tally_launch, reduce_steps
        rew, info, done = env.last_rewards[None], env.last_info_words[None], dones["__all__"][None]
        if self.device.type != "cuda":
            self.stats.copy_(reduce_steps(rew, info, done, self.layout, stats=self.stats))
            self.wstats.copy_(world_tally_reference(info, self.wstats))
            return
        _tally_launch(rew, info, done.view(torch.uint8) if done.dtype == torch.bool else done, self._masks,
                      self.layout.info_words, self.stats)
        _world_launch(info, self.wstats)


def _mean_std(n: float, s: float, s2: float) -> Dict[str, float]:
    """mean and population standard deviation of n values with sum s and sum of squares s2 (NaN for n = 0)"""
    from ..evaluate import _mean_std as ms
    return ms(n, s, s2)


class TrainDiag:
    """An update's diagnostics (``metrics["diag"]`` under ``TRAIN_DIAG``): clones of the update's accumulators,
    so that a later graph replay does not overwrite them, read (copied to the host) only when asked.

    stats: float64 [E, n_agents, EVAL_WORDS], ``reduce_steps`` over the update's steps; wstats: float64
    [E, WORLD_TALLY_WORDS]; words: per agent type the float64 [DIAG_WORDS] of :func:`rollout_diag`; nvecs: per
    type the heads' widths; multi: per type whether the action space is MultiDiscrete; type_names: the agent
    types' names (``env.type_names``).  A mean over zero values is NaN."""

    def __init__(self, stats: torch.Tensor, wstats: torch.Tensor, words: Sequence[torch.Tensor], layout,
                 nvecs: Sequence[Sequence[int]], multi: Sequence[bool], type_names: Sequence[str]):
        self._stats_t, self.wstats = stats.clone(), wstats.clone()
        self.words = [w.clone() for w in words]
        self.layout, self.nvecs, self.multi = layout, [list(n) for n in nvecs], list(multi)
        self.type_names = list(type_names)
        self.n_types = len(self.words)
        self._stats = None
        self._host: Dict[int, List[float]] = {}

    @property
    def stats(self):
        """the update's ``evaluate.EvalStats`` (rewards, info fields, episodes) over its steps"""
        if self._stats is None:
            from ..evaluate import EvalStats
            self._stats = EvalStats(self._stats_t, self.layout)
        return self._stats

    def _w(self, t: int) -> List[float]:
        if t not in self._host:
            self._host[t] = self.words[t].cpu().tolist()
        return self._host[t]

    def world(self) -> Dict[str, Dict[str, float]]:
        """every world info field over the update's env steps: {name: {"mean", "std"}} by ``layout.INFO_WORLD``"""
        from ..evaluate import W_STEPS
        n = float(self._stats_t[:, 0, W_STEPS].sum().item())      # the envs' steps (agent 0 counts them)
        tot = self.wstats.sum(dim=0).cpu().tolist()
        return {name: _mean_std(n, tot[2 * k], tot[2 * k + 1]) for k, (name, _) in enumerate(INFO_WORLD)}

    def actions(self, t: int) -> List[Dict]:
        """per head of type t: ``shares`` (percent of the N action words, per action), ``mean`` (of the in-range
        words) and ``out_of_range`` (the count of words in no bin)"""
        w = self._w(t)
        n, heads = w[D_N], []
        for k, nk in enumerate(self.nvecs[t]):
            bins = w[D_ACT_BIN + DIAG_MAX_ACTIONS * k:D_ACT_BIN + DIAG_MAX_ACTIONS * k + nk]
            inr = n - w[D_ACT_OOR + k]
            heads.append({"shares": [100.0 * b / n if n > 0 else math.nan for b in bins],
                          "mean": w[D_ACT_SUM + k] / inr if inr > 0 else math.nan,
                          "out_of_range": int(w[D_ACT_OOR + k])})
        return heads

    def moments(self, t: int) -> Dict:
        """mean and std of type t's reward, value, log_prob, advantage and target over the rollout,
        ``explained_variance`` = 1 - Var(target - value) / Var(target) from population variances (NaN when
        Var(target) <= 0 or the rollout is empty) and ``dones`` (the set global-done elements)"""
        w = self._w(t)
        n = w[D_N]
        out = {name: _mean_std(n, w[D_Q + 2 * q], w[D_Q + 2 * q + 1]) for q, name in enumerate(QUANTITIES[:5])}

        def var(q):
            m = w[D_Q + 2 * q] / n
            return w[D_Q + 2 * q + 1] / n - m * m

        ev = math.nan
        if n > 0 and var(4) > 0:
            ev = 1.0 - max(var(5), 0.0) / var(4)
        out["explained_variance"] = ev
        out["dones"] = int(w[D_DONES])
        return out

    def summary(self) -> Dict[str, float]:
        """One flat dict for the log, the reference's keys where it has them: ``agent_{name}/{field}_mean`` and
        ``_std`` of every agent info field, ``agent_{name}/action_{a}`` (percent) for a Discrete type or
        ``agent_{name}/action_dim_{k}_mean_quant`` for a MultiDiscrete one, ``world/{key}_mean``; and
        ``agent_{name}/episodes``, ``episode_reward_mean``, ``episode_length_mean``, ``explained_variance``,
        ``value_mean`` and ``advantage_std``."""
        out: Dict[str, float] = {}
        st = self.stats
        for t, name in enumerate(self.type_names):
            p = f"agent_{name}/"
            for field, ms in st.info(t).items():
                out[f"{p}{field}_mean"], out[f"{p}{field}_std"] = ms["mean"], ms["std"]
            heads = self.actions(t)
            if self.multi[t]:
                for k, h in enumerate(heads):
                    out[f"{p}action_dim_{k}_mean_quant"] = h["mean"]
            else:
                for a, share in enumerate(heads[0]["shares"]):
                    out[f"{p}action_{a}"] = share
            mo = self.moments(t)
            out[f"{p}episodes"] = st.episodes(t)
            out[f"{p}episode_reward_mean"] = st.episode_reward(t)["mean"]
            out[f"{p}episode_length_mean"] = st.episode_length(t)["mean"]
            out[f"{p}explained_variance"] = mo["explained_variance"]
            out[f"{p}value_mean"] = mo["value"]["mean"]
            out[f"{p}advantage_std"] = mo["advantage"]["std"]
        for key, ms in self.world().items():
            out[f"world/{key}_mean"] = ms["mean"]
        return out


__all__ = ["rollout_diag", "rollout_diag_reference", "world_tally", "world_tally_reference", "RolloutTally",
           "TrainDiag", "diag_supported", "diag_workspace", "stripe_rows", "stripes", "QUANTITIES", "DIAG_WORDS",
           "WORLD_TALLY_WORDS"]
