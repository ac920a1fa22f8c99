"""Fixed-action baseline evaluation: the reference's
gymnax_exchange/jaxrl/MARL/baseline_eval/baseline_only_JAXMARL.py (reset NUM_ENVS envs, step them
NUM_STEPS times with one FixedAction per agent type, report the trajectory batch as a few numbers)
on :meth:`MARLEnv.rollout_eval`, whose persistent launch folds every step's rewards and info words
into per-agent accumulators instead of writing a trajectory.

* :func:`reduce_steps` is the accumulators' definition, a sequential float64 loop over per-step
  outputs in torch: what the kernel is held to (bit for bit), and the way in for someone who
  already holds per-step outputs.
* :class:`EvalStats` names the accumulator words (include/hftlob.h lists them) and turns them
  into counts, means and population standard deviations per agent type.
* :func:`evaluate_fixed_actions` is the script's loop; ``python -m hftlob.evaluate`` prints its
  numbers as one JSON object.
* :func:`tally_steps` is :func:`reduce_steps` as one HIP launch (hftlob_eval_tally), bit for bit.
* :func:`evaluate_policy` is the same loop with the recurrent policies of a checkpoint
  (``hftlob.train.ippo.load_policy``) in place of the fixed actions, for all agent types or, with a
  fixed action for the others, for some: one fused policy step per learned type and one env step per
  step, each step tallied from the env's output buffers with :func:`tally_steps`
  (``python -m hftlob.evaluate --checkpoint PATH``).
* :func:`evaluate_combinations` runs every learned / baseline mix per agent type under one seed, the
  reference's baseline_eval/baseline_JAXMARL.py (``BB``, ``BL``, ``LB``, ``LL`` for two types;
  ``--checkpoint PATH --baseline-actions 4,2 --combinations``).  The reference's per-combination
  agent-config overrides (BASELINE_CONFIGS, get_ma_config) are not covered: one env config serves
  every combination.
* :class:`Uniform` is the reference's stochastic baseline as a policy entry: its FixedAction with
  several actions (one of them drawn uniformly at every step) and, as ``Uniform.all()``, its
  RandomPolicy (baseline_JAXMARL.py:367-394).  :func:`draw_actions_reference` defines the draw in
  numpy, :func:`draw_actions` is its launch (hftlob_draw_actions), :func:`evaluate_baseline` is
  :func:`evaluate_fixed_actions` for fixed and drawn types in any mix, drawing inside the persistent
  launch (``--uniform-actions 1+2+3,all``); :func:`evaluate_policy` and
  :func:`evaluate_combinations` take a ``Uniform`` where they take a fixed action.

* Per-episode records: the launches above also write one record per (env, agent, completed episode)
  into an ``episodes`` buffer (``max_episodes=`` / ``episodes=``; include/hftlob.h lists the words), and
  :class:`EpisodeLog` reads it: the episode rewards ``[episodes, agents]``, lengths and end-of-episode
  info fields, their quantiles, tail means and histograms, and ``EpisodeLog.save`` /
  :func:`save_combinations` write the files baseline_eval/plotting_combinations.py loads
  (``--episodes-out PATH``).

Plotting itself (the rest of baseline_eval/) is not covered.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import EPISODE_WORDS, EVAL_WORDS
from .layout import AGENT_MM, INFO_AGENT_WORDS, INFO_EXE, INFO_MM, INFO_WORLD_WORDS

# words of an agent's row (include/hftlob.h, hftlob_env_rollout_eval)
W_STEPS, W_EPISODES, W_RUN_SUM, W_RUN_LEN, W_EP_SUM, W_EP_SUM2, W_EP_LEN, W_EP_LEN2 = range(8)
W_STEP_Q = 8            # + 2q, + 2q + 1: quantity q (0 the reward, 1 + k info word k) over all steps
W_END_INFO = 58         # + 2k, + 2k + 1: info word k at each episode's last step
N_QUANT = 1 + INFO_AGENT_WORDS
assert W_STEP_Q + 2 * N_QUANT == W_END_INFO and W_END_INFO + 2 * INFO_AGENT_WORDS == EVAL_WORDS
# words of an episode's record (include/hftlob.h, hftlob_env_rollout_eval_episodes)
R_SUM, R_LEN, R_INFO = 0, 1, 2      # the reward sum, the length, + k: info word k at the last step
assert R_INFO + INFO_AGENT_WORDS == EPISODE_WORDS


def _float_words(layout) -> torch.Tensor:
    """bool [n_agents, INFO_AGENT_WORDS]: the float32 words of each agent's info block."""
    rows = []
    for kind in layout.agent_kinds:
        fields = INFO_MM if kind == AGENT_MM else INFO_EXE
        rows.append([bool(isf) for _, isf in fields] + [False] * (INFO_AGENT_WORDS - len(fields)))
    return torch.tensor(rows, dtype=torch.bool)


def _check_cap(cap) -> int:
    if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1:
        raise ValueError(f"max_episodes (ep_cap) must be an int >= 1, got {cap!r}")
    return cap


def reduce_steps(rewards, info_words: torch.Tensor, done_all: torch.Tensor, layout,
                 stats: Optional[torch.Tensor] = None, episodes: Optional[torch.Tensor] = None,
                 max_episodes: Optional[int] = None):
    """The accumulators of hftlob_env_rollout_eval from per-step outputs, as a sequential float64
    loop over the steps (every word is one plain sum in step order; a widened float32 / int32
    squares exactly), on the inputs' device.

    rewards: float32 [T, E, n_agents], or the per-type list ``rollout(per_step=True)`` returns.
    info_words: the raw info record, int32 [T, E, info_words] (``env.last_info_words`` of a
    per_step rollout, reshaped; [T * E, info_words] is accepted).  done_all: bool [T, E].
    layout: the env's ``EnvLayout``.  stats: float64 [E, n_agents, EVAL_WORDS] to continue from
    (not modified); None starts from zeros.  Returns the new stats tensor.

    With ``max_episodes`` (the cap) or ``episodes`` (float64 [E, n_agents, cap, EPISODE_WORDS] to continue
    from, not modified; with the cap alone it starts from zeros) the per-episode records are kept as
    well, and the return value is ``(stats, episodes)``.  At a step whose done_all is set, agent a's
    record is the running reward sum and length as they are added to words 4 and 6, then the step's 24
    info words as they are added to words 58 + 2k; it goes to slot i = word 1 before the step's
    increment, iff 0 <= i < cap.  Every other slot keeps what it held.  This is the definition the HIP
    launches are held to bit for bit."""
    if not isinstance(rewards, torch.Tensor):
        rewards = torch.cat([x.reshape(x.shape[0], x.shape[1], -1) for x in rewards], dim=2)
    T, E, A = rewards.shape
    if A != len(layout.agent_kinds) or rewards.dtype != torch.float32:
        raise ValueError(f"rewards must be float32 [T, E, {len(layout.agent_kinds)}]")
    if info_words.dtype != torch.int32 or info_words.numel() != T * E * layout.info_words:
        raise ValueError(f"info_words must be int32 [T, E, {layout.info_words}]")
    if tuple(done_all.shape) != (T, E):
        raise ValueError("done_all must be [T, E]")
    dev = rewards.device
    st = torch.zeros((E, A, EVAL_WORDS), dtype=torch.float64, device=dev) if stats is None else stats.clone()
    if tuple(st.shape) != (E, A, EVAL_WORDS) or st.dtype != torch.float64 or st.device != dev:
        raise ValueError(f"stats must be float64 [{E}, {A}, {EVAL_WORDS}] on {dev}")
    ep = None
    if episodes is not None or max_episodes is not None:
        if episodes is not None and (not isinstance(episodes, torch.Tensor) or episodes.dim() != 4):
            raise ValueError(f"episodes must be float64 [{E}, {A}, cap, {EPISODE_WORDS}] on {dev}")
        cap = _check_cap(max_episodes if max_episodes is not None else int(episodes.shape[2]))
        ep = torch.zeros((E, A, cap, EPISODE_WORDS), dtype=torch.float64, device=dev) if episodes is None \
            else episodes.clone()
        if tuple(ep.shape) != (E, A, cap, EPISODE_WORDS) or ep.dtype != torch.float64 or ep.device != dev:
            raise ValueError(f"episodes must be float64 [{E}, {A}, {cap}, {EPISODE_WORDS}] on {dev}")
    iw = info_words.reshape(T, E, layout.info_words)[:, :, INFO_WORLD_WORDS:INFO_WORLD_WORDS + A * INFO_AGENT_WORDS]
    iw = iw.reshape(T, E, A, INFO_AGENT_WORDS).contiguous()
    isf = _float_words(layout).to(dev)
    x = torch.empty((T, E, A, N_QUANT), dtype=torch.float64, device=dev)
    x[..., 0] = rewards.to(torch.float64)
    x[..., 1:] = torch.where(isf, iw.view(torch.float32).to(torch.float64), iw.to(torch.float64))
    x2 = x * x
    done = done_all.to(device=dev, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for t in range(T):
        d = done[t][:, None]                                   # [E, 1] over the agents
        if ep is not None:
            # the record of every (env, agent) whose episode ends here, at the count before this step
            i = st[:, :, W_EPISODES]
            w = d & (i >= 0) & (i < cap)                       # [E, A]
            rec = torch.cat([(st[:, :, W_RUN_SUM] + x[t, :, :, 0])[..., None], (st[:, :, W_RUN_LEN] + 1.0)[..., None],
                             x[t, :, :, 1:]], dim=2)           # [E, A, EPISODE_WORDS]
            e_i, a_i = torch.nonzero(w, as_tuple=True)
            ep[e_i, a_i, i[e_i, a_i].to(torch.int64)] = rec[e_i, a_i]
        st[:, :, W_STEPS] += 1.0
        st[:, :, W_EPISODES] += d.to(torch.float64)
        run_sum = st[:, :, W_RUN_SUM] + x[t, :, :, 0]
        run_len = st[:, :, W_RUN_LEN] + 1.0
        for w, v in ((W_EP_SUM, run_sum), (W_EP_SUM2, run_sum * run_sum), (W_EP_LEN, run_len),
                     (W_EP_LEN2, run_len * run_len)):
            st[:, :, w] = torch.where(d, st[:, :, w] + v, st[:, :, w])
        st[:, :, W_RUN_SUM] = torch.where(d, zero, run_sum)
        st[:, :, W_RUN_LEN] = torch.where(d, zero, run_len)
        st[:, :, W_STEP_Q:W_END_INFO:2] += x[t]
        st[:, :, W_STEP_Q + 1:W_END_INFO:2] += x2[t]
        d3 = d[:, :, None]
        st[:, :, W_END_INFO::2] = torch.where(d3, st[:, :, W_END_INFO::2] + x[t, :, :, 1:], st[:, :, W_END_INFO::2])
        st[:, :, W_END_INFO + 1::2] = torch.where(d3, st[:, :, W_END_INFO + 1::2] + x2[t, :, :, 1:],
                                                  st[:, :, W_END_INFO + 1::2])
    return st if ep is None else (st, ep)


def _float_word_masks(layout):
    """:func:`_float_words` as hftlob_eval_tally's host array: uint32 [n_agents], bit k = word k is a float"""
    rows = _float_words(layout).tolist()
    return (C.c_uint32 * len(rows))(*[sum(1 << k for k, isf in enumerate(r) if isf) for r in rows])


def _tally_launch(rewards, info_words, done_all, masks, info_w: int, stats, episodes=None) -> None:
    """hftlob_eval_tally on checked device tensors ([T, E, A], [T, E, info_w], [T, E] bytes), adding to stats;
    with ``episodes`` ([E, A, cap, EPISODE_WORDS]) hftlob_eval_tally_episodes, which also writes the records"""
    T, E, A = rewards.shape
    dev = rewards.device
    with torch.cuda.device(dev):
        if episodes is None:
            _lib.check(_lib.lib().hftlob_eval_tally(E, A, T, info_w, _lib.ptr(rewards), _lib.ptr(info_words),
                                                    _lib.ptr(done_all), masks, _lib.ptr(stats),
                                                    _lib.stream_ptr(device=dev)))
        else:
            _lib.check(_lib.lib().hftlob_eval_tally_episodes(E, A, T, info_w, _lib.ptr(rewards), _lib.ptr(info_words),
                                                             _lib.ptr(done_all), masks, _lib.ptr(stats),
                                                             _lib.ptr(episodes), int(episodes.shape[2]),
                                                             _lib.stream_ptr(device=dev)))


def _check_episodes(episodes, E: int, A: int, dev) -> None:
    """a caller's ``episodes`` buffer of a launch: contiguous float64 [E, A, cap >= 1, EPISODE_WORDS] on dev"""
    if (not isinstance(episodes, torch.Tensor) or episodes.dtype != torch.float64 or episodes.dim() != 4
            or tuple(episodes.shape[:2]) != (E, A) or episodes.shape[3] != EPISODE_WORDS or episodes.shape[2] < 1
            or episodes.device != dev or not episodes.is_contiguous()):
        raise ValueError(f"episodes must be a contiguous float64 [{E}, {A}, cap, {EPISODE_WORDS}] tensor on {dev} "
                         "with cap (ep_cap) >= 1")


def tally_steps(rewards, info_words: torch.Tensor, done_all: torch.Tensor, layout,
                stats: Optional[torch.Tensor] = None, episodes: Optional[torch.Tensor] = None):
    """:func:`reduce_steps` as one launch of hftlob_eval_tally (csrc/eval_tally.hip) on torch's current
    stream: the same arguments, the same bits.  The tensors must be on a GPU (there is no other path);
    done_all is bool or uint8 [T, E].  Unlike reduce_steps a given ``stats`` (contiguous float64
    [E, n_agents, EVAL_WORDS] on that device) is continued IN PLACE; None starts from zeros.  Returns
    the stats tensor.  Nothing is allocated beyond a missing ``stats`` and a per-type rewards list's
    concatenation, and nothing synchronises.
    episodes: a contiguous float64 [E, n_agents, cap, EPISODE_WORDS] tensor on that device for the
    per-episode records (hftlob_eval_tally_episodes; :func:`reduce_steps` defines them), filled IN PLACE;
    the return value is then ``(stats, episodes)``."""
    if not isinstance(rewards, torch.Tensor):
        rewards = torch.cat([x.reshape(x.shape[0], x.shape[1], -1) for x in rewards], dim=2)
    if rewards.dim() != 3 or rewards.shape[2] != len(layout.agent_kinds) or rewards.dtype != torch.float32:
        raise ValueError(f"rewards must be float32 [T, E, {len(layout.agent_kinds)}]")
    T, E, A = rewards.shape
    if T < 1 or E < 1:
        raise ValueError("tally_steps needs at least one step and one env")
    if not isinstance(info_words, torch.Tensor) or info_words.dtype != torch.int32 \
            or info_words.numel() != T * E * layout.info_words:
        raise ValueError(f"info_words must be int32 [T, E, {layout.info_words}]")
    if not isinstance(done_all, torch.Tensor) or tuple(done_all.shape) != (T, E) \
            or done_all.dtype not in (torch.bool, torch.uint8):
        raise ValueError("done_all must be bool or uint8 [T, E]")
    dev = rewards.device
    if dev.type != "cuda" or info_words.device != dev or done_all.device != dev:
        raise ValueError(f"tally_steps needs its tensors on one GPU device, got {dev}, {info_words.device} and "
                         f"{done_all.device}")
    if stats is None:
        stats = torch.zeros((E, A, EVAL_WORDS), dtype=torch.float64, device=dev)
    elif (not isinstance(stats, torch.Tensor) or tuple(stats.shape) != (E, A, EVAL_WORDS) or stats.dtype != torch.float64
          or stats.device != dev or not stats.is_contiguous()):
        raise ValueError(f"stats must be a contiguous float64 [{E}, {A}, {EVAL_WORDS}] tensor on {dev}")
    if episodes is not None:
        _check_episodes(episodes, E, A, dev)
    if done_all.dtype == torch.bool:
        done_all = done_all.view(torch.uint8)
    _tally_launch(rewards.contiguous(), info_words.contiguous(), done_all.contiguous(), _float_word_masks(layout),
                  layout.info_words, stats, episodes)
    return stats if episodes is None else (stats, episodes)


def _mean_std(n: float, s: float, s2: float) -> Dict[str, float]:
    """mean and population standard deviation of n values with sum s and sum of squares s2
    (NaN for n = 0; a variance that rounds below 0 counts as 0)."""
    if n <= 0:
        return {"mean": math.nan, "std": math.nan}
    m = s / n
    return {"mean": m, "std": math.sqrt(max(s2 / n - m * m, 0.0))}


class EvalStats:
    """A stats tensor (float64 [E, n_agents, EVAL_WORDS]) read per agent type.  Reductions over
    the envs and a type's agents are plain float64 sums of the accumulator words; a mean or
    standard deviation over zero values is NaN."""

    def __init__(self, stats: torch.Tensor, layout):
        if stats.dim() != 3 or stats.shape[1] != len(layout.agent_kinds) or stats.shape[2] != EVAL_WORDS \
                or stats.dtype != torch.float64:
            raise ValueError(f"stats must be float64 [E, {len(layout.agent_kinds)}, {EVAL_WORDS}]")
        self.stats = stats
        self.layout = layout
        self.n_types = max(layout.agent_types) + 1
        self._tot = [stats[:, [a for a, t in enumerate(layout.agent_types) if t == i]].sum(dim=(0, 1)).cpu().tolist()
                     for i in range(self.n_types)]

    def fields(self, t: int) -> List[str]:
        """the info field names of type t (layout.INFO_MM / INFO_EXE)"""
        kind = self.layout.agent_kinds[self.layout.agent_types.index(t)]
        return [n for n, _ in (INFO_MM if kind == AGENT_MM else INFO_EXE)]

    def steps(self, t: int) -> int:
        """agent-steps tallied (envs x agents of the type x steps)"""
        return int(self._tot[t][W_STEPS])

    def episodes(self, t: int) -> int:
        """episodes completed, counted per agent of the type"""
        return int(self._tot[t][W_EPISODES])

    def total_dones(self) -> int:
        """the envs' global dones (the reference's total_dones: done["__all__"] summed)"""
        return int(self.stats[:, 0, W_EPISODES].sum().item())

    def _q(self, t: int, n: float, w: int) -> Dict[str, float]:
        return _mean_std(n, self._tot[t][w], self._tot[t][w + 1])

    def reward(self, t: int) -> Dict[str, float]:
        return self._q(t, self._tot[t][W_STEPS], W_STEP_Q)

    def info(self, t: int) -> Dict[str, Dict[str, float]]:
        """every info field over all steps"""
        return {n: self._q(t, self._tot[t][W_STEPS], W_STEP_Q + 2 * (1 + k)) for k, n in enumerate(self.fields(t))}

    def info_at_episode_end(self, t: int) -> Dict[str, Dict[str, float]]:
        """every info field at the episodes' last steps"""
        return {n: self._q(t, self._tot[t][W_EPISODES], W_END_INFO + 2 * k) for k, n in enumerate(self.fields(t))}

    def episode_reward(self, t: int) -> Dict[str, float]:
        """the completed episodes' reward sums"""
        return self._q(t, self._tot[t][W_EPISODES], W_EP_SUM)

    def episode_length(self, t: int) -> Dict[str, float]:
        return self._q(t, self._tot[t][W_EPISODES], W_EP_LEN)

    def summary(self) -> dict:
        """The numbers baseline_only_JAXMARL.py prints and logs, per agent type."""
        types = []
        for t in range(self.n_types):
            r = self.reward(t)
            types.append({"avg_reward": r["mean"], "std_reward": r["std"], "steps": self.steps(t),
                          "episodes": self.episodes(t), "info": self.info(t),
                          "episode_reward": self.episode_reward(t), "episode_length": self.episode_length(t),
                          "info_at_episode_end": self.info_at_episode_end(t)})
        return {"total_dones": self.total_dones(), "types": types}


class EpisodeLog:
    """The per-episode records of an evaluation read as arrays: ``episodes`` (float64 [E, n_agents, cap,
    EPISODE_WORDS], as the launches or :func:`reduce_steps` filled it from zeroed ``stats``) with the
    ``stats`` tensor that counts them.  Env e completed ``stats[e, 0, 1]`` episodes (all agents of an env
    share done_all, so they share the count), of which the first ``cap`` have a record; the others were
    dropped.  A row of the arrays below is one episode: the (env, episode index) pairs in env-major
    order.  ``t`` is an agent type; a type's values are those of all its agents.  Everything is float64
    on the CPU."""

    def __init__(self, episodes: torch.Tensor, stats: torch.Tensor, layout):
        A = len(layout.agent_kinds)
        if not isinstance(episodes, torch.Tensor) or episodes.dim() != 4 or episodes.shape[1] != A \
                or episodes.shape[3] != EPISODE_WORDS or episodes.dtype != torch.float64:
            raise ValueError(f"episodes must be float64 [E, {A}, cap, {EPISODE_WORDS}]")
        E, cap = int(episodes.shape[0]), int(episodes.shape[2])
        if not isinstance(stats, torch.Tensor) or tuple(stats.shape) != (E, A, EVAL_WORDS) or stats.dtype != torch.float64:
            raise ValueError(f"stats must be float64 [{E}, {A}, {EVAL_WORDS}]")
        self.layout = layout
        self.cap = cap
        self.n_types = max(layout.agent_types) + 1
        done = stats[:, 0, W_EPISODES].cpu().to(torch.int64)
        self.count = done.clamp(0, cap)                                   # [E]: episodes with a record
        self.dropped = int((done - self.count).clamp(min=0).sum().item())   # completed, but past the cap
        keep = torch.arange(cap)[None, :] < self.count[:, None]           # [E, cap]
        self._rec = episodes.cpu().permute(0, 2, 1, 3)[keep]              # [n_episodes, A, EPISODE_WORDS]
        self.env = torch.nonzero(keep, as_tuple=True)[0]                  # [n_episodes]: each row's env

    def __len__(self) -> int:
        return int(self._rec.shape[0])

    def _agents(self, t: int) -> List[int]:
        ags = [a for a, ty in enumerate(self.layout.agent_types) if ty == t]
        if not ags:
            raise ValueError(f"no agent type {t}")
        return ags

    def fields(self, t: int) -> List[str]:
        """the info field names of type t (layout.INFO_MM / INFO_EXE)"""
        kind = self.layout.agent_kinds[self._agents(t)[0]]
        return [n for n, _ in (INFO_MM if kind == AGENT_MM else INFO_EXE)]

    def rewards(self) -> torch.Tensor:
        """the episodes' reward sums [n_episodes, n_agents]: plotting_combinations.py's array of a configuration"""
        return self._rec[:, :, R_SUM].clone()

    def lengths(self) -> torch.Tensor:
        """the episodes' lengths in steps [n_episodes] (the agents of an env share them)"""
        return self._rec[:, 0, R_LEN].clone()

    def field(self, t: int, name: str) -> torch.Tensor:
        """info field ``name`` of type t at the episodes' last steps [n_episodes, the type's agents]"""
        names = self.fields(t)
        if name not in names:
            raise ValueError(f"agent type {t} has no info field {name!r}; its fields: {names}")
        return self._rec[:, self._agents(t), R_INFO + names.index(name)].clone()

    def values(self, t: int, what: str = "reward") -> torch.Tensor:
        """type t's values of ``what`` over all episodes and the type's agents, flat: "reward" (the
        episode's reward sum), "length", or an info field at the episode's last step"""
        if what == "reward":
            return self._rec[:, self._agents(t), R_SUM].reshape(-1)
        if what == "length":
            return self._rec[:, self._agents(t), R_LEN].reshape(-1)
        return self.field(t, what).reshape(-1)

    def quantiles(self, t: int, qs: Sequence[float], what: str = "reward") -> torch.Tensor:
        """``torch.quantile`` (linear interpolation) of the values in float64, [len(qs)]; NaN without episodes"""
        v = self.values(t, what)
        q = torch.as_tensor(list(qs), dtype=torch.float64)
        if v.numel() == 0:
            return torch.full_like(q, math.nan)
        return torch.quantile(v, q)

    def cvar(self, t: int, alpha: float, what: str = "reward") -> float:
        """the mean of the worst (smallest) ``alpha`` share of the values: the ceil(alpha n) smallest of
        n, at least one (the expected shortfall of the episode outcome); NaN without episodes"""
        if not 0.0 < alpha <= 1.0:
            raise ValueError(f"alpha must be in (0, 1], got {alpha}")
        v = self.values(t, what)
        if v.numel() == 0:
            return math.nan
        k = min(v.numel(), max(1, math.ceil(alpha * v.numel() - 1e-12)))
        return float(torch.sort(v)[0][:k].mean().item())

    def histogram(self, t: int, bins: int = 30, what: str = "reward") -> Tuple[torch.Tensor, torch.Tensor]:
        """(counts float64 [bins], edges float64 [bins + 1]) of the finite values, ``bins`` equal bins
        between their minimum and maximum (the plots' ``hist(all_rewards, bins=30)``)"""
        v = self.values(t, what)
        v = v[torch.isfinite(v)]
        if v.numel() == 0:
            return torch.zeros(bins, dtype=torch.float64), torch.linspace(0.0, 1.0, bins + 1, dtype=torch.float64)
        return tuple(torch.histogram(v, bins=bins))

    def summary(self, qs: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95), alpha: float = 0.05) -> dict:
        """a JSON-able digest: the counts, and per agent type the episode reward's mean, extremes,
        quantiles and tail mean, and the episode length's mean"""
        types = []
        for t in range(self.n_types):
            r = self.values(t, "reward")
            n = int(r.numel())
            qv = self.quantiles(t, qs).tolist()
            types.append({"values": n,
                          "episode_reward": {"mean": float(r.mean().item()) if n else math.nan,
                                             "min": float(r.min().item()) if n else math.nan,
                                             "max": float(r.max().item()) if n else math.nan,
                                             "quantiles": {str(q): v for q, v in zip(qs, qv)},
                                             "cvar": {"alpha": alpha, "value": self.cvar(t, alpha)}},
                          "episode_length": {"mean": float(self.values(t, "length").mean().item()) if n else math.nan}})
        return {"episodes": len(self), "dropped": self.dropped, "cap": self.cap, "types": types}

    def save(self, path: str, name: str = "Config") -> None:
        """The episode rewards as configuration ``name`` of a file baseline_eval/plotting_combinations.py
        loads; the format follows the suffix (.npz, .json, .pkl, .csv; :func:`save_combinations` has the
        formats)."""
        _save_reward_arrays(path, {name: self.rewards().numpy()})


def _agent_columns(n_agents: int) -> List[str]:
    """the CSV's agent columns: the reference's two names for two agents, Agent_i otherwise"""
    return ["MarketMaker", "ExecutionAgent"] if n_agents == 2 else [f"Agent_{i}" for i in range(n_agents)]


def _save_reward_arrays(path: str, arrays: Dict[str, np.ndarray]) -> None:
    """{name: float64 [episodes, agents]} in the formats baseline_eval/plotting_combinations.py loads, by
    the path's suffix: .npz (one array per name), .json (nested lists per name), .pkl (the pickled dict of
    arrays), .csv (a row per name and episode: Configuration, Episode, then a column per agent)."""
    suffix = os.path.splitext(path)[1].lower()
    if suffix == ".npz":
        with open(path, "wb") as f:          # (a file object: numpy appends no second suffix)
            np.savez(f, **arrays)
    elif suffix == ".json":
        with open(path, "w") as f:
            json.dump({k: v.tolist() for k, v in arrays.items()}, f)
    elif suffix == ".pkl":
        import pickle
        with open(path, "wb") as f:
            pickle.dump(dict(arrays), f)
    elif suffix == ".csv":
        import csv
        with open(path, "w", newline="") as f:
            wr = csv.writer(f)
            cols = None
            for name, arr in arrays.items():
                if cols is None:
                    cols = _agent_columns(arr.shape[1])
                    wr.writerow(["Configuration", "Episode"] + cols)
                elif len(cols) != arr.shape[1]:
                    raise ValueError("the configurations of one CSV file must have the same number of agents")
                for i, row in enumerate(arr):
                    wr.writerow([name, i] + [repr(float(x)) for x in row])
            if cols is None:
                wr.writerow(["Configuration", "Episode"])
    else:
        raise ValueError(f"episodes file {path!r}: the suffix must be .npz, .json, .pkl or .csv")


def save_combinations(path: str, logs: Dict[str, EpisodeLog]) -> None:
    """:func:`evaluate_combinations`' logs {desc: EpisodeLog} as the configurations ``Config_<desc>``
    (Config_BB, Config_BL, Config_LB, Config_LL for two types) of one such file."""
    _save_reward_arrays(path, {f"Config_{desc}": log.rewards().numpy() for desc, log in logs.items()})


MAX_DRAW_ACTIONS = 32   # the actions of a drawn type: one 32-bit mask, one lane per action


def _several_fixed_actions(t: int, n: int) -> NotImplementedError:
    return NotImplementedError(
        f"agent type {t}: {n} fixed actions; the reference draws one of them uniformly per step "
        "(JAX's categorical), which is not implemented for a bare list: give one action per agent type, or "
        "Uniform([...]) for the draw")


@dataclass(frozen=True)
class Uniform:
    """A policy entry: at every step each agent of the type takes one of ``actions``, drawn uniformly
    (:func:`draw_actions_reference` is the draw).  ``Uniform([1, 2, 3])`` is the reference's
    FixedAction with several actions (baseline_eval/baseline_only_JAXMARL.py:58-71),
    ``Uniform.all()`` its RandomPolicy (baseline_JAXMARL.py:367-374): every action of the type's space,
    filled in when the entry meets an env.  ``Uniform([a])`` is the fixed action ``a``."""
    actions: Optional[Tuple[int, ...]]

    def __post_init__(self):
        if self.actions is None:
            return
        if isinstance(self.actions, (str, bytes)) or not isinstance(self.actions, Iterable):
            raise TypeError(f"Uniform: actions must be a list of ints, got {type(self.actions).__name__}")
        acts = tuple(self.actions)
        if not acts:
            raise ValueError("Uniform: an empty list of actions (Uniform.all() is every action of the space)")
        for a in acts:
            if isinstance(a, bool) or not isinstance(a, int):
                raise TypeError(f"Uniform: an action must be an int, got {type(a).__name__} {a!r}")
            if a < 0:
                raise ValueError(f"Uniform: a negative action {a}")
        if len(set(acts)) != len(acts):
            raise ValueError(f"Uniform: duplicate actions in {list(acts)} (a weighted set is not covered)")
        object.__setattr__(self, "actions", acts)

    @classmethod
    def all(cls) -> "Uniform":
        return cls(None)

    def mask(self, n_actions: int) -> int:
        """the allowed set in a space of ``n_actions`` as a bit mask (bit a = action a)"""
        if self.actions is None:
            return (1 << n_actions) - 1
        for a in self.actions:
            if a >= n_actions:
                raise ValueError(f"Uniform: action {a} is outside the type's {n_actions} actions")
        return sum(1 << a for a in self.actions)

    def spelling(self) -> str:
        """the command line's form: ``all``, or the actions joined with ``+``"""
        return "all" if self.actions is None else "+".join(str(a) for a in self.actions)


def masked_first_argmax(noise: np.ndarray, allowed: int):
    """Per row of ``noise`` (float32 [B, A]) the smallest a with bit a of ``allowed`` set that maximises
    noise[b, a]; returns (int32 [B], float32 [B]: the gap between the row's two largest allowed noises,
    inf where one action is allowed)."""
    noise = np.asarray(noise, dtype=np.float32)
    A = noise.shape[1]
    live = np.array([bool((allowed >> a) & 1) for a in range(A)])
    if not live.any() or allowed >> A:
        raise ValueError(f"allowed {allowed:#x} must be a non-empty mask of bits < {A}")
    score = np.where(live[None, :], noise, -np.inf).astype(np.float32)
    top = score.max(axis=1, keepdims=True)
    actions = np.where(score == top, np.arange(A)[None, :], A).min(axis=1).astype(np.int32)
    if live.sum() < 2:
        return actions, np.full(noise.shape[0], np.inf, dtype=np.float32)
    two = np.sort(score, axis=1)[:, -2:]
    return actions, (two[:, 1] - two[:, 0]).astype(np.float32)


def _check_draw(n_actors: int, n_actions: int, allowed: int) -> None:
    if n_actors < 1:
        raise ValueError("n_actors must be >= 1")
    if not 1 <= n_actions <= MAX_DRAW_ACTIONS:
        raise ValueError(f"n_actions must be 1..{MAX_DRAW_ACTIONS}, got {n_actions}")
    if allowed <= 0 or allowed >> n_actions:
        raise ValueError(f"allowed {allowed:#x} must be a non-empty mask of bits < {n_actions}")


def draw_actions_reference(key, n_actors: int, n_actions: int, allowed: int):
    """The draw of a uniform baseline policy, in numpy: actor b takes the smallest a with bit a of
    ``allowed`` set that maximises g[b, a], g = jax.random.gumbel(key, (n_actors, n_actions)) under the
    partitionable threefry in float32 (``train.policy.gumbel_noise``: the word of counter
    (0, b n_actions + a)), which is jax.random.categorical on logits 0 on the allowed actions and -inf
    elsewhere.  A mask of one bit draws nothing.  Returns (actions int32 [n_actors], gaps float32
    [n_actors]): a row's gap is the distance between its two largest allowed noises; a device's float32
    logarithm may round a last place differently, so tests hold only rows with a clear gap."""
    from .train.policy import gumbel_noise
    _check_draw(n_actors, n_actions, allowed)
    if allowed & (allowed - 1) == 0:
        return (np.full(n_actors, allowed.bit_length() - 1, dtype=np.int32),
                np.full(n_actors, np.inf, dtype=np.float32))
    return masked_first_argmax(gumbel_noise(key, n_actors, n_actions).numpy(), allowed)


def _draw_launch(n_actors: int, n_actions: int, allowed: int, key: torch.Tensor, out: torch.Tensor) -> None:
    """hftlob_draw_actions on checked device tensors (key [2], out int32 [n_actors] in any shape)"""
    dev = out.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hftlob_draw_actions(n_actors, n_actions, allowed, _lib.ptr(key), _lib.ptr(out),
                                                  _lib.stream_ptr(device=dev)))


def draw_actions(key: torch.Tensor, n_actors: int, n_actions: int, allowed: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`draw_actions_reference`'s actions as one launch of hftlob_draw_actions
    (csrc/draw_actions.hip) on torch's current stream.  key: uint32 / int32 [2] on a GPU (there is no
    other path); out: a contiguous int32 [n_actors] tensor on that device to fill, None allocates one.
    Nothing else is allocated and nothing synchronises."""
    _check_draw(n_actors, n_actions, allowed)
    if not isinstance(key, torch.Tensor) or key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2 \
            or not key.is_contiguous():
        raise ValueError("key must be a contiguous uint32/int32 tensor of two words")
    if key.device.type != "cuda":
        raise ValueError(f"draw_actions needs its key on a GPU device, got {key.device}")
    if out is None:
        out = torch.empty(n_actors, dtype=torch.int32, device=key.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.numel() != n_actors
          or out.device != key.device or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int32 [{n_actors}] tensor on {key.device}")
    _draw_launch(n_actors, n_actions, allowed, key, out)
    return out


def draw_masks(env, entries: Sequence, fixed_too: bool = False) -> List[Optional[int]]:
    """The allowed masks of checked policy entries (:func:`policy_entries`) on ``env``, one per agent
    type: a :class:`Uniform`'s set in the type's space and None for the others, or with ``fixed_too``
    (every type goes through the draw: :func:`evaluate_baseline`) a fixed action's one bit as well.
    A type with a mask needs a Discrete space of at most 32 actions, and a :class:`Uniform` the env's
    partitionable keys.  Host-only: nothing of the device is touched."""
    masks: List[Optional[int]] = []
    for t, (p, wd, sp) in enumerate(zip(entries, env.action_widths, env.action_spaces)):
        if isinstance(p, torch.nn.Module) or (isinstance(p, int) and not fixed_too):
            masks.append(None)
            continue
        if wd != 1 or not isinstance(sp.n, int):
            raise ValueError(f"agent type {t}: a drawn baseline needs a Discrete action space, the type's is "
                             f"MultiDiscrete ({wd} words per agent)")
        if sp.n > MAX_DRAW_ACTIONS:
            raise ValueError(f"agent type {t}: a drawn baseline covers at most {MAX_DRAW_ACTIONS} actions, the "
                             f"type has {sp.n}")
        if isinstance(p, Uniform):
            try:
                masks.append(p.mask(sp.n))
            except ValueError as e:
                raise ValueError(f"agent type {t}: {e}") from None
        else:
            if not 0 <= p < sp.n:
                raise ValueError(f"agent type {t}: action {p} is outside the type's {sp.n} actions")
            masks.append(1 << p)
    if any(m is not None for m in masks) and not bool(env.cfg_c.prng_partitionable):
        raise ValueError("a drawn baseline is built for the partitionable threefry only: the env has "
                         "prng_partitionable off")
    return masks


def fixed_action_row(env, fixed_actions: Sequence) -> torch.Tensor:
    """FIXED_ACTIONS (one entry per agent type: an int, or a list of one int as the reference's
    configs write it) -> the int32 [action_words] row of ``rollout_eval(fixed=True)``: every agent
    of a type, and every word of a MultiDiscrete space, takes the type's action."""
    counts = env.multi_agent_config.number_of_agents_per_type
    if len(fixed_actions) != len(counts):
        raise ValueError(f"fixed_actions must hold one entry per agent type ({len(counts)}), got {len(fixed_actions)}")
    row = []
    for t, (a, n, wd) in enumerate(zip(fixed_actions, counts, env.action_widths)):
        if isinstance(a, (list, tuple)):
            if len(a) != 1:
                raise _several_fixed_actions(t, len(a))
            a = a[0]
        row += [int(a)] * (n * wd)
    return torch.tensor(row, dtype=torch.int32, device=env.device)


def eval_keys(rng: torch.Tensor, n_envs: int, n_steps: int, partitionable: bool):
    """n_steps of the script's step-key chain from the carried key ``rng`` (int32 [1, 2], device):
    per step ``rng, _ = split(rng)`` (the unused action sample) and ``rng, _rng = split(rng)``, then
    ``split(_rng, n_envs)`` for all the steps at once.  Returns (rng', keys [n_steps, n_envs, 2])."""
    from .env import split_keys
    rng, sub, _ = _key_chain(rng, n_steps, partitionable)
    return rng, split_keys(torch.cat(sub).contiguous(), n_envs, partitionable)


def _key_chain(rng: torch.Tensor, n_steps: int, partitionable: bool):
    """The chain of :func:`eval_keys`: (rng', each step's ``_rng`` [1, 2], each step's action-sample
    key [1, 2]: the second key of the step's first split, which a fixed-action run leaves unused)."""
    from .env import split_keys
    sub, act = [], []
    for _ in range(n_steps):
        first = split_keys(rng, 2, partitionable)
        rng = first[:, 0].contiguous()
        act.append(first[:, 1])
        pair = split_keys(rng, 2, partitionable)
        rng = pair[:, 0].contiguous()
        sub.append(pair[:, 1])
    return rng, sub, act


def _new_episodes(env, n_envs: int, max_episodes: Optional[int]) -> Optional[torch.Tensor]:
    """the zeroed records buffer of an evaluation with ``max_episodes`` (None: no records)"""
    if max_episodes is None:
        return None
    return torch.zeros((n_envs, len(env.layout.agent_kinds), _check_cap(max_episodes), EPISODE_WORDS),
                       dtype=torch.float64, device=env.device)


def evaluate_fixed_actions(env, fixed_actions: Sequence, n_envs: int, n_steps: int, seed: int,
                           chunk: int = 256, max_episodes: Optional[int] = None):
    """baseline_only_JAXMARL.py's evaluation: reset ``n_envs`` envs, step them ``n_steps`` times
    with one fixed action per agent type, and reduce.  The keys follow the shape of the script's
    chain from ``PRNGKey(seed)``: ``rng, _rng = split(rng)`` and ``split(_rng, n_envs)`` for the
    reset, then :func:`eval_keys` per step, generated ``chunk`` steps at a time on the device; one
    ``rollout_eval(fixed=True)`` launch per chunk carries the stats over.  Returns the
    :class:`EvalStats`; with ``max_episodes`` the launches also keep each env's first ``max_episodes``
    episodes' records, in one buffer carried across the chunks, and the return value is
    ``(EvalStats, EpisodeLog)``."""
    from .env import split_keys
    if n_envs < 1 or n_steps < 1 or chunk < 1:
        raise ValueError("n_envs, n_steps and chunk must be >= 1")
    row = fixed_action_row(env, fixed_actions)
    part = bool(env.cfg_c.prng_partitionable)
    params = env.default_params
    rng = torch.tensor([[0, int(seed) & 0xFFFFFFFF]], dtype=torch.int64).to(torch.int32).to(env.device)
    pair = split_keys(rng, 2, part)
    rng = pair[:, 0].contiguous()
    _, state = env.reset(split_keys(pair[:, 1].contiguous(), n_envs, part)[0], params)
    stats = None
    episodes = _new_episodes(env, n_envs, max_episodes)
    for t0 in range(0, n_steps, chunk):
        rng, keys = eval_keys(rng, n_envs, min(chunk, n_steps - t0), part)
        stats = env.rollout_eval(keys, state, row, params, stats=stats, fixed=True, episodes=episodes)[5]
    if episodes is None:
        return EvalStats(stats, env.layout)
    return EvalStats(stats, env.layout), EpisodeLog(episodes, stats, env.layout)


def evaluate_baseline(env, entries: Sequence, n_envs: int, n_steps: int, seed: int, chunk: int = 256,
                      max_episodes: Optional[int] = None):
    """:func:`evaluate_fixed_actions` for baselines that draw: ``entries`` holds one int, list of one
    int or :class:`Uniform` per agent type, in any mix, and one ``rollout_eval_drawn`` launch per
    chunk draws every type's actions inside the env launch (a fixed action is a mask of one bit, which
    draws nothing).  The reset and step keys are that function's chain unchanged; type i's draw key at
    a step is ``split(act, n_types)[i]`` of the key the chain leaves unused (:func:`_key_chain`), what
    :func:`evaluate_policy` hands the type, so the two give the same stats for the same entries.  Every
    type needs a Discrete space of at most 32 actions, and a :class:`Uniform` partitionable keys.
    ``max_episodes``: as :func:`evaluate_fixed_actions` takes it (the return value becomes
    ``(EvalStats, EpisodeLog)``; the records are the same for the same entries too)."""
    from .env import split_keys
    if n_envs < 1 or n_steps < 1 or chunk < 1:
        raise ValueError("n_envs, n_steps and chunk must be >= 1")
    n_types = len(env.multi_agent_config.number_of_agents_per_type)
    pols = policy_entries(entries, n_types)
    for t, p in enumerate(pols):
        if isinstance(p, torch.nn.Module):
            raise TypeError(f"agent type {t}: evaluate_baseline takes fixed actions and Uniform entries; a network "
                            "goes through evaluate_policy")
    allowed = draw_masks(env, pols, fixed_too=True)
    part = bool(env.cfg_c.prng_partitionable)
    params = env.default_params
    rng = torch.tensor([[0, int(seed) & 0xFFFFFFFF]], dtype=torch.int64).to(torch.int32).to(env.device)
    pair = split_keys(rng, 2, part)
    rng = pair[:, 0].contiguous()
    _, state = env.reset(split_keys(pair[:, 1].contiguous(), n_envs, part)[0], params)
    stats = None
    episodes = _new_episodes(env, n_envs, max_episodes)
    for t0 in range(0, n_steps, chunk):
        rng, sub, act = _key_chain(rng, min(chunk, n_steps - t0), part)
        keys = split_keys(torch.cat(sub).contiguous(), n_envs, part)                      # [T, E, 2]
        draw_keys = split_keys(torch.cat(act).contiguous(), n_types, part)                # [T, n_types, 2]
        stats = env.rollout_eval_drawn(keys, state, draw_keys, allowed, params, stats=stats, episodes=episodes)[5]
    if episodes is None:
        return EvalStats(stats, env.layout)
    return EvalStats(stats, env.layout), EpisodeLog(episodes, stats, env.layout)


def _fixed_action(t: int, a) -> int:
    """one type's fixed action as :func:`fixed_action_row` reads it: an int, or a list of one int"""
    if isinstance(a, (list, tuple)):
        if len(a) != 1:
            raise _several_fixed_actions(t, len(a))
        a = a[0]
    if isinstance(a, bool) or not isinstance(a, int):
        raise TypeError(f"agent type {t}: a policy entry must be an ActorCriticRNN, a Uniform, an int or a list of "
                        f"one int, got {type(a).__name__}")
    return a


def policy_entries(nets: Sequence, n_types: int) -> list:
    """The entries of :func:`evaluate_policy`'s ``nets`` checked, one per agent type: a network (any
    ``torch.nn.Module``; an ``ActorCriticRNN`` is what runs) and a :class:`Uniform` stay, a fixed
    action (an int, or a list of one int as the reference's FIXED_ACTIONS writes it) becomes its int.
    Host-only."""
    if len(nets) != n_types:
        raise ValueError(f"nets must hold one network or fixed action per agent type ({n_types}), got {len(nets)}")
    return [p if isinstance(p, (torch.nn.Module, Uniform)) else _fixed_action(t, p) for t, p in enumerate(nets)]


def evaluate_policy(env, nets, n_envs: int, n_steps: int, seed: int, greedy: bool = True,
                    chunk: int = 64, grouped: bool = False, max_episodes: Optional[int] = None):
    """:func:`evaluate_fixed_actions` with recurrent policies in place of the fixed actions: ``nets``
    holds one entry per agent type, an ``ActorCriticRNN`` (``hftlob.train.ippo.load_policy``) or a
    fixed action (an int, or a list of one int), in any mix.  Every agent of a fixed type, and every
    action word of a MultiDiscrete one, takes that action at every step; the type has no carry and no
    policy launch.  The reset and the env step keys are that function's chain unchanged; the key its
    chain leaves unused each step (:func:`eval_keys`' "unused action sample") is the step's policy key,
    split once more per agent type whatever the mix, so a learned type draws the same samples
    whichever other types are fixed.  Each step is one fused policy step per learned type
    (``train.policy.policy_step_net``: the argmax if ``greedy``, else a ``jax.random.categorical``
    sample per head), followed by ``env.step`` and one :func:`tally_steps` launch over the env's own
    output buffers (rewards, raw info words, global dones): nothing is copied or kept per step.  The
    carries start at zero and are reset by each actor's done.  ``chunk`` sizes the key generation
    only.  The env must be built with ``return_info=True``.
    An entry may also be a :class:`Uniform`: the type (a Discrete space of at most 32 actions) has no
    carry either, and its step is one :func:`draw_actions` launch under the type's policy key of the
    step, the key a learned type would sample with; learned and fixed types are as without it.
    ``grouped``: the learned types' steps of a step are one launch (``train.policy.policy_step_grouped``: at
    most 8 learned types of one FC_DIM_SIZE and GRU_HIDDEN_DIM), with the same statistics bit for bit.
    ``max_episodes``: every step's tally launch also writes the records of the episodes that end there
    (hftlob_eval_tally_episodes) into one buffer, and the return value is ``(EvalStats, EpisodeLog)``."""
    from .env import split_keys
    from .train.policy import GREEDY, SAMPLE, policy_step_grouped, policy_step_grouped_supported, policy_step_net
    if n_envs < 1 or n_steps < 1 or chunk < 1:
        raise ValueError("n_envs, n_steps and chunk must be >= 1")
    if not getattr(env, "return_info", False):
        raise ValueError("evaluate_policy reduces the steps' info words: build the env with return_info=True")
    counts = list(env.multi_agent_config.number_of_agents_per_type)
    pols = policy_entries(nets, len(counts))
    learned = [i for i, p in enumerate(pols) if isinstance(p, torch.nn.Module)]
    if grouped and learned and not policy_step_grouped_supported([pols[i] for i in learned]):
        raise ValueError("evaluate_policy(grouped=True) needs at most 8 learned types of one FC_DIM_SIZE and "
                         "GRU_HIDDEN_DIM, each within the fused policy step's sizes")
    drawn = [i for i, p in enumerate(pols) if isinstance(p, Uniform)]
    allowed = draw_masks(env, pols) if drawn else None
    part = bool(env.cfg_c.prng_partitionable)
    params, dev, E, L = env.default_params, env.device, n_envs, env.layout
    mode = GREEDY if greedy else SAMPLE
    rng = torch.tensor([[0, int(seed) & 0xFFFFFFFF]], dtype=torch.int64).to(torch.int32).to(dev)
    pair = split_keys(rng, 2, part)
    rng = pair[:, 0].contiguous()
    obs, state = env.reset(split_keys(pair[:, 1].contiguous(), n_envs, part)[0], params)
    n_act = [n * E for n in counts]
    # a fixed type's action words, built once: [E, n_t * width]
    actions = [torch.full((E, n * wd), p, dtype=torch.int32, device=dev) if isinstance(p, int) else None
               for p, n, wd in zip(pols, counts, env.action_widths)]
    for i in drawn:   # a drawn type's action words [E, n_t], refilled by its draw at every step
        actions[i] = torch.empty((E, counts[i]), dtype=torch.int32, device=dev)
    obs = {i: obs[i].reshape(n_act[i], -1).contiguous() for i in learned}
    done = {i: torch.zeros(n_act[i], dtype=torch.bool, device=dev) for i in learned}
    h = {i: torch.zeros(n_act[i], pols[i].hidden, device=dev) for i in learned}
    masks = _float_word_masks(L)
    A = len(L.agent_kinds)
    stats = torch.zeros((E, A, EVAL_WORDS), dtype=torch.float64, device=dev)
    episodes = _new_episodes(env, E, max_episodes)
    for t0 in range(0, n_steps, chunk):
        T = min(chunk, n_steps - t0)
        rng, sub, act = _key_chain(rng, T, part)
        keys = split_keys(torch.cat(sub).contiguous(), n_envs, part)                       # [T, E, 2]
        pol = split_keys(torch.cat(act).contiguous(), len(pols), part)                     # [T, n_types, 2]
        for t in range(T):
            if grouped and learned:
                outs = policy_step_grouped([pols[i] for i in learned], [obs[i] for i in learned],
                                           [done[i] for i in learned], [h[i] for i in learned], mode,
                                           keys=[pol[t, i] for i in learned] if mode == SAMPLE else None)
            for j, i in enumerate(learned):
                a = outs[j][1] if grouped else policy_step_net(pols[i], obs[i], done[i], h[i], mode,
                                                               key=pol[t, i] if mode == SAMPLE else None)[1]
                actions[i] = a.view(E, counts[i], *a.shape[1:])   # [E, n_t], or [E, n_t, K] of a MultiDiscrete type
            for i in drawn:
                _draw_launch(n_act[i], env.action_spaces[i].n, allowed[i], pol[t, i], actions[i])
            o, state, _, d, _ = env.step(keys[t], state, actions, params)
            # the step's raw outputs where the env launch wrote them: [E, A], [E, info_words], [E]
            _tally_launch(env.last_rewards.view(1, E, A), env.last_info_words.view(1, E, L.info_words),
                          d["__all__"].view(torch.uint8).view(1, E), masks, L.info_words, stats, episodes)
            for i in learned:
                obs[i] = o[i].reshape(n_act[i], -1).contiguous()
                done[i] = d["agents"][i].reshape(-1).contiguous()
    if episodes is None:
        return EvalStats(stats, L)
    return EvalStats(stats, L), EpisodeLog(episodes, stats, L)


def combination_names(n_types: int) -> List[str]:
    """The reference's names of the 2^n learned / baseline mixes in its order (binary counting, one
    character per agent type, 'L' for 1 and 'B' for 0): BB, BL, LB, LL for two types."""
    if n_types < 1:
        raise ValueError("n_types must be >= 1")
    return ["".join("L" if (c >> (n_types - 1 - t)) & 1 else "B" for t in range(n_types)) for c in range(2 ** n_types)]


def mix_entries(desc: str, nets: Sequence, fixed_actions: Sequence) -> list:
    """:func:`evaluate_policy`'s ``nets`` of one mix: type t's network where ``desc[t]`` is 'L', its
    fixed action where it is 'B'."""
    if len(desc) != len(nets) or len(desc) != len(fixed_actions) or set(desc) - set("LB"):
        raise ValueError(f"a mix is one 'L' or 'B' per agent type ({len(nets)} nets, {len(fixed_actions)} fixed "
                         f"actions), got {desc!r}")
    return [n if c == "L" else a for c, n, a in zip(desc, nets, fixed_actions)]


def evaluate_combinations(env, nets, fixed_actions: Sequence, n_envs: int, n_steps: int, seed: int,
                          greedy: bool = True, max_episodes: Optional[int] = None) -> dict:
    """baseline_JAXMARL.py's evaluation (:819-951): every combination of the learned policy
    (``nets[t]``) and the baseline (``fixed_actions[t]``) per agent type through
    :func:`evaluate_policy`, all under the same seed, so the runs are paired as the reference's are
    (it passes the same rng to each).  Returns {name: EvalStats} in :func:`combination_names`' order.
    One env config serves all combinations (the reference's per-combination agent configs are not
    covered).  With ``max_episodes`` the values are ``(EvalStats, EpisodeLog)``
    (:func:`save_combinations` writes the logs as the reference's plots read them)."""
    n = len(env.multi_agent_config.number_of_agents_per_type)
    policy_entries(nets, n)
    policy_entries(fixed_actions, n)
    return {desc: evaluate_policy(env, mix_entries(desc, nets, fixed_actions), n_envs, n_steps, seed, greedy=greedy,
                                  max_episodes=max_episodes)
            for desc in combination_names(n)}


def parse_entries(text: str) -> list:
    """The command line's baseline entries, one per agent type, comma-separated: an int (a fixed
    action), a ``+``-joined set (``1+2+3``: :class:`Uniform` over it) or ``all`` (``Uniform.all()``)."""
    out = []
    for item in text.split(","):
        item = item.strip()
        if item == "all":
            out.append(Uniform.all())
        elif "+" in item:
            out.append(Uniform([int(x) for x in item.split("+")]))
        else:
            out.append(int(item))
    return out


def entry_spelling(p):
    """a baseline entry as :func:`parse_entries` reads it (an int stays an int)"""
    return p.spelling() if isinstance(p, Uniform) else p


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m hftlob.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--env-config", required=True, help="a built-in config name, or the path of a config .json")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--fixed-actions",
                      help="one action per agent type, comma-separated (the reference's FIXED_ACTIONS)")
    what.add_argument("--uniform-actions", metavar="1+2+3,all",
                      help="one entry per agent type, comma-separated: a '+'-joined set drawn uniformly at every step "
                           "(the reference's FixedAction with several actions), a single action, or 'all' (its "
                           "RandomPolicy)")
    what.add_argument("--checkpoint", metavar="PATH",
                      help="evaluate the policies of an IPPOTrainer checkpoint (python -m hftlob.train.ippo --save)")
    ap.add_argument("--sample", action="store_true",
                    help="with --checkpoint: sample the actions (jax.random.categorical) instead of the argmax")
    ap.add_argument("--baseline-actions", metavar="A,B",
                    help="with --checkpoint: one fixed action per agent type for the types a mix runs as baseline "
                         "(or a drawn entry, as --uniform-actions spells it)")
    ap.add_argument("--combinations", action="store_true",
                    help="with --baseline-actions: every learned / baseline mix per agent type (BB, BL, LB, LL)")
    ap.add_argument("--mix", metavar="LB",
                    help="with --baseline-actions: one mix, 'L' (learned) or 'B' (baseline) per agent type")
    ap.add_argument("--envs", type=int, required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=None,
                    help="steps per launch (default 256), or with --checkpoint per key generation (default 64)")
    ap.add_argument("--data-msgs", type=int, default=400_000, help="length of the synthetic message day")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--episodes-out", metavar="PATH",
                    help="write the episode rewards [episodes, agents] to PATH as the reference's "
                         "plotting_combinations.py loads them (.npz, .json, .pkl or .csv by the suffix); the JSON "
                         "object gains the records' digest")
    ap.add_argument("--max-episodes", type=int, default=128,
                    help="with --episodes-out: the records kept per env (default 128); later episodes are counted as "
                         "dropped")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.sample and not args.checkpoint:
        ap.error("--sample needs --checkpoint")
    if args.baseline_actions and not args.checkpoint:
        ap.error("--baseline-actions needs --checkpoint")
    if (args.combinations or args.mix) and not args.baseline_actions:
        ap.error("--combinations and --mix need --baseline-actions")
    if args.baseline_actions and bool(args.combinations) == bool(args.mix):
        ap.error("--baseline-actions takes one of --combinations and --mix")
    from .config_io import builtin_config, load_config_from_file
    from .data.synthetic import generate_day
    from .env import MARLEnv
    cfg = load_config_from_file(args.env_config) if os.path.exists(args.env_config) else builtin_config(args.env_config)
    cap = None
    if args.episodes_out:
        if os.path.splitext(args.episodes_out)[1].lower() not in (".npz", ".json", ".pkl", ".csv"):
            ap.error("--episodes-out: the suffix must be .npz, .json, .pkl or .csv")
        if args.max_episodes < 1:
            ap.error("--max-episodes must be >= 1")
        cap = args.max_episodes

    def finish(out: dict, ev) -> int:
        """one evaluation's JSON line; with --episodes-out also its records file and digest"""
        if cap is not None:
            ev, log = ev
        out.update(ev.summary())
        if cap is not None:
            log.save(args.episodes_out)
            out["episodes"] = log.summary()
            out["episodes_dropped"] = log.dropped
        print(json.dumps(out))
        return 0

    w = cfg.world_config
    day = generate_day(n_msgs=args.data_msgs, snap_every=w.n_data_msg_per_step * w.start_resolution)
    if args.checkpoint:
        from .train.ippo import load_policy
        env = MARLEnv(None, cfg, data=day, device=args.device, return_info=True, persistent_outputs=True)
        nets = load_policy(args.checkpoint, env, args.device)
        if args.baseline_actions:
            base = parse_entries(args.baseline_actions)
            out = {"env_config": args.env_config, "checkpoint": args.checkpoint, "sample": bool(args.sample),
                   "baseline_actions": [entry_spelling(p) for p in base], "envs": args.envs, "steps": args.steps,
                   "seed": args.seed}
            if args.combinations:
                evs = evaluate_combinations(env, nets, base, args.envs, args.steps, args.seed, greedy=not args.sample,
                                            max_episodes=cap)
            else:
                evs = {args.mix: evaluate_policy(env, mix_entries(args.mix, nets, base), args.envs, args.steps,
                                                 args.seed, greedy=not args.sample, chunk=args.chunk or 64,
                                                 max_episodes=cap)}
            if cap is not None:
                logs = {desc: log for desc, (_, log) in evs.items()}
                evs = {desc: ev for desc, (ev, _) in evs.items()}
            out["combinations"] = {desc: ev.summary() for desc, ev in evs.items()}
            if cap is not None:
                save_combinations(args.episodes_out, logs)
                out["episodes"] = {desc: log.summary() for desc, log in logs.items()}
                out["episodes_dropped"] = sum(log.dropped for log in logs.values())
            print(json.dumps(out))
            return 0
        ev = evaluate_policy(env, nets, args.envs, args.steps, args.seed, greedy=not args.sample,
                             chunk=args.chunk or 64, max_episodes=cap)
        out = {"env_config": args.env_config, "checkpoint": args.checkpoint, "sample": bool(args.sample),
               "envs": args.envs, "steps": args.steps, "seed": args.seed}
        return finish(out, ev)
    env = MARLEnv(None, cfg, data=day, device=args.device, return_info=False, persistent_outputs=True)
    if args.uniform_actions:
        entries = parse_entries(args.uniform_actions)
        ev = evaluate_baseline(env, entries, args.envs, args.steps, args.seed, args.chunk or 256, max_episodes=cap)
        out = {"env_config": args.env_config, "uniform_actions": [entry_spelling(p) for p in entries],
               "envs": args.envs, "steps": args.steps, "seed": args.seed}
        return finish(out, ev)
    actions = [int(x) for x in args.fixed_actions.split(",")]
    ev = evaluate_fixed_actions(env, actions, args.envs, args.steps, args.seed, args.chunk or 256, max_episodes=cap)
    out = {"env_config": args.env_config, "fixed_actions": actions, "envs": args.envs, "steps": args.steps,
           "seed": args.seed}
    return finish(out, ev)


if __name__ == "__main__":
    sys.exit(main())
