"""IPPO with recurrent actor-critics, trained against the HIP env step (the
reference's consumer loop, gymnax_exchange/jaxrl/MARL/ippo_rnn_JAXMARL.py).

One network (and optimizer) per agent type, as the reference:

* ``ActorCriticRNN`` (:203-256): Dense(FC_DIM_SIZE, orthogonal sqrt 2) + relu ->
  GRU(GRU_HIDDEN_DIM) whose carry is zeroed where the actor's previous done is set
  (ScannedRNN, :53-78) -> critic Dense(FC)+relu+Dense(1) and actor
  Dense(GRU_HIDDEN_DIM)+relu+Dense(n_actions, orthogonal 0.01) categorical head
  (SingleActionOutput :183-201); for a MultiDiscrete space one such head per action word
  (MultiActionOutputIndependant :80-100) under MultiCategorical (:259-281: the sample stacks the
  heads' samples, log_prob and entropy are the sums over the heads), as EXE ``fixed_prices`` needs.
* rollout (:578-663): NUM_STEPS steps of sample -> env.step, the transitions kept
  in preallocated device buffers (no host synchronisation inside the rollout);
  actors are (env, agent) pairs of one type, ``batchify`` order.
* GAE (:668-690) with the per-type GAMMA / GAE_LAMBDA and the env's global done.
* PPO update (:711-838): UPDATE_EPOCHS x NUM_MINIBATCHES over a permutation of
  the actors (whole sequences, the GRU is re-run from the rollout's initial carry);
  clipped value loss, clipped surrogate with per-minibatch advantage
  normalisation, entropy bonus; Adam(eps 1e-5) after global-norm clipping, linear
  LR annealing by update count.
* multi-GPU (ippo_rnn_JAXMARL_pmap.py:566-567 pmean of grads): every rank steps
  its own env shard; gradients are averaged with one all-reduce per agent type
  and minibatch (``torch.distributed``, RCCL on ROCm).

On the GPU each minibatch step (forward over the sequence, loss, backward,
clipping, Adam) is captured once per step group (an agent type, or with
``GROUPED_SCAN`` all of them) in a HIP graph and replayed
(``CUDA_GRAPHS``, single-process runs): a 64-step GRU unroll is thousands of small
kernels, and replaying them as one graph removes their launch cost.

Differences that are not semantics of the env: action sampling and parameter
initialisation draw from torch's generator, not JAX's threefry, and the network
runs through torch (rocBLAS GEMMs) rather than XLA.  With ``FUSED_POLICY`` the rollout's
policy step is one HIP launch per agent type and step (``train.policy.policy_step``) and its
samples are ``jax.random.categorical`` draws from a carried threefry key, so nothing inside the
rollout reads torch's generator.  With ``GROUPED_POLICY`` (on top of ``FUSED_POLICY``) a rollout step's
policy steps of all the agent types are one launch (``train.policy.policy_step_grouped``), bit for bit the per-type
launches; ``train.population.PopulationTrainer`` trains several independent runs of one env config in lockstep on it.
With ``FUSED_LOSS`` the update's GAE is one HIP launch and the
minibatch step's loss with its gradient three (``train.loss.gae``, ``train.loss.ppo_loss_fused``).
With ``FUSED_OPT`` the minibatch step's clipping and Adam step are two HIP launches per agent type
(``train.optim.adam_clip_step``) on capturable Adam's state, so the checkpoints do not change.
With ``GROUPED_SCAN`` (on top of ``FUSED_GRU``) the agent types' minibatch steps run in lockstep as one
joint step whose sequence scans are one HIP launch per direction for all the types
(``train.gru.gru_scan_grouped``): the nets and their data are independent, so every parameter, optimiser
state and metric is bit for bit what the per-type steps give.
With ``FUSED_WGRAD`` the weight and bias gradients of the narrow layers (``embed``, ``actor2``, ``critic2``) are
two HIP launches each (``train.wgrad.narrow_linear``: a reduction split over the minibatch's rows) instead of
rocBLAS GEMMs that run on a handful of workgroups; the forward, the data gradients and the square layers stay
with rocBLAS, and parameters, ``state_dict`` and checkpoints are untouched.
``FUSED_WGRAD_WIDE`` does the same, independently, for the wide layers (the GRU's ``weight_ih``, ``actor1``,
``critic1``: ``train.wgrad.wide_linear``, the product on the matrix cores), and with ``FUSED_GRU`` for the
GRU's ``weight_hh`` (``train.gru.weight_grads_fused``, which also drops the concatenations and the select that
built its operands).
With ``TRAIN_DIAG`` (an env built with ``return_info="raw"``) every rollout step's rewards, info record and global
done are folded into per-agent and per-env accumulators on the device (``train.diag.RolloutTally``: the evaluation
tally and a world tally, inside the captured rollout), after GAE each agent type's buffers are reduced to a few
words (``train.diag.rollout_diag``), and ``metrics["diag"]`` is the update's ``train.diag.TrainDiag``: the action
shares, info means and stds, episode counts and explained variance the reference's update callback (:977-1059)
logs.  It reads what the update wrote and writes only tensors of its own, so training is bit for bit what it is
without it.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..env import MARLEnv, split_keys
from .gru import MAX_GROUPS, SUPPORTED_HIDDEN, gru_scan, gru_scan_grouped, gru_scan_supported
from .loss import gae as gae_fused, ppo_loss_fused, ppo_loss_supported
from .optim import MAX_TENSORS, adam_clip_step, adam_clip_supported, init_adam_state
from .diag import (DIAG_MAX_ACTIONS, DIAG_MAX_HEADS, DIAG_WORDS, RolloutTally, TrainDiag, diag_supported, diag_workspace,
                   rollout_diag, rollout_diag_reference)
from .policy import (MAX_ACTIONS, MAX_GROUPS as MAX_POLICY_GROUPS, MAX_HEADS, MAX_OBS_DIM, SAMPLE, policy_step_grouped,
                     policy_step_multi_supported, policy_step_net)
from .wgrad import MAX_P, SUPPORTED_Q, narrow_linear, narrow_linear_supported, wide_linear, wide_linear_supported


def _per_type(v, n: int) -> list:
    """A per-agent-type hyper-parameter list of length n (a scalar or a shorter list repeats its last value)."""
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * n)[:n]


@dataclass(frozen=True)
class Switch:
    """One on/off key of the config (default off).  The trainer carries its value as the attribute
    ``key.lower()``, and ``main`` takes it as the command-line flag ``flag``."""
    key: str
    help: str           # the flag's help text
    gpu: bool = True    # the trainer refuses the switch on any other device (there is no other path behind it)
    # what a net the switch cannot take is told, without the "(agent type i)" that the trainer appends; else None
    check: Optional[Callable[["ActorCriticRNN", Dict], Optional[str]]] = None

    @property
    def flag(self) -> str:
        return "--" + self.key.lower().replace("_", "-")


def _policy_step_check(lead: str):
    """The per-net check of a switch that runs the fused policy step (``train.policy``); ``lead`` opens its text."""
    def check(n, c):
        D = n.embed.in_features
        if policy_step_multi_supported(D, c["FC_DIM_SIZE"], c["GRU_HIDDEN_DIM"], n.heads):
            return None
        return (f"{lead} GRU_HIDDEN_DIM and FC_DIM_SIZE in {list(SUPPORTED_HIDDEN)}, an observation size <= "
                f"{MAX_OBS_DIM} and <= {MAX_ACTIONS} actions (in each of <= {MAX_HEADS} heads), got "
                f"{c['GRU_HIDDEN_DIM']}, {c['FC_DIM_SIZE']}, {D} and {n.heads}")
    return check


def _loss_check(n, c):
    if not ppo_loss_supported(n.heads):
        return f"FUSED_LOSS needs <= {MAX_ACTIONS} actions (in each of <= {MAX_HEADS} heads), got {n.heads}"


def _opt_check(n, c):
    if not adam_clip_supported(len(list(n.parameters()))):
        return f"FUSED_OPT needs <= {MAX_TENSORS} parameter tensors in a net, got {len(list(n.parameters()))}"


def _wgrad_check(n, c):
    if not all(narrow_linear_supported(m.in_features, m.out_features) for m in (n.embed, n.actor2, n.critic2)):
        return (f"FUSED_WGRAD needs GRU_HIDDEN_DIM and FC_DIM_SIZE in {list(SUPPORTED_Q)}, an observation size <= "
                f"{MAX_P} and <= {MAX_P} actions over all heads, got {c['GRU_HIDDEN_DIM']}, {c['FC_DIM_SIZE']}, "
                f"{n.embed.in_features} and {sum(n.heads)}")


def _wgrad_wide_check(n, c):
    sizes = ((n.gru.input_size, 3 * n.hidden), (n.hidden, 3 * n.hidden), (n.actor1.in_features, n.actor1.out_features),
             (n.critic1.in_features, n.critic1.out_features))
    if not all(wide_linear_supported(i, o) for i, o in sizes):
        return (f"FUSED_WGRAD_WIDE needs GRU_HIDDEN_DIM and FC_DIM_SIZE in {list(SUPPORTED_Q)}, got "
                f"{c['GRU_HIDDEN_DIM']} and {c['FC_DIM_SIZE']}")


def _diag_check(n, c):
    if not diag_supported(n.heads):
        return (f"TRAIN_DIAG needs <= {DIAG_MAX_ACTIONS} actions (in each of <= {DIAG_MAX_HEADS} heads), got "
                f"{n.heads}")


# Every switch, in the order the trainer checks them.  The module docstring says what each one does; what a
# switch needs beyond a device and a per-net check (FUSED_GRU's hidden size and its CPU rule, GROUPED_SCAN's
# three conditions, CALC_EVAL's eval env, TRAIN_DIAG's env mode) is in IPPOTrainer.__init__.
SWITCHES = [
    Switch("FUSED_GRU", "the PPO update's GRU scan as the fused HIP operators", gpu=False),   # on the CPU: the loop
    Switch("FUSED_POLICY", "the rollout's policy step, sample and log-prob as one fused HIP launch",
           check=_policy_step_check("FUSED_POLICY needs")),
    Switch("GROUPED_POLICY", "the agent types' policy steps of a rollout step as one fused HIP launch (needs "
           "--fused-policy)", check=_policy_step_check("GROUPED_POLICY needs")),
    Switch("FUSED_LOSS", "the update's GAE and PPO loss (with its gradient) as fused HIP launches", check=_loss_check),
    Switch("FUSED_OPT", "the minibatch step's global-norm clip and Adam step as two fused HIP launches",
           check=_opt_check),
    Switch("GROUPED_SCAN", "the agent types' minibatch steps in lockstep, their GRU scans one HIP launch per direction "
           "(needs --fused-gru)", gpu=False),   # FUSED_GRU's device rule: on the CPU the scans are the loops
    Switch("FUSED_WGRAD", "the narrow layers' (embed, actor2, critic2) weight and bias gradients as two fused HIP "
           "launches each", check=_wgrad_check),
    Switch("FUSED_WGRAD_WIDE", "the wide layers' (the GRU's two weight matrices, actor1, critic1) weight and bias "
           "gradients as two fused HIP launches each", check=_wgrad_wide_check),
    Switch("CALC_EVAL", "CALC_EVAL: after every update NUM_STEPS_EVAL sampled steps in a separate eval env (the same "
           "config, a synthetic day of another seed), logged as avg_reward_eval",
           check=_policy_step_check("CALC_EVAL runs the fused policy step: it needs")),
    Switch("TRAIN_DIAG", "per-update diagnostics tallied on the device (action shares, info means and stds, episodes, "
           "explained variance), logged as diag; the env is built with return_info='raw'", gpu=False,
           check=_diag_check),   # on the CPU: train.diag's reference functions
]


def default_config(**kw) -> Dict:
    """The reference's ippo_rnn_JAXMARL_2player.yaml hyper-parameters (training keys only), every switch off."""
    c = {"LR": [2.5e-4, 2.5e-4], "NUM_ENVS": 4096, "NUM_STEPS": 64, "GRU_HIDDEN_DIM": 256, "FC_DIM_SIZE": 256,
         "TOTAL_TIMESTEPS": 5e8, "UPDATE_EPOCHS": 4, "NUM_MINIBATCHES": 4, "GAMMA": [0.999999999, 0.999],
         "GAE_LAMBDA": [0.85, 0.9], "CLIP_EPS": 0.2, "ENT_COEF": [0.01, 0.01], "VF_COEF": [0.5, 0.5],
         "MAX_GRAD_NORM": [0.5, 0.5], "ANNEAL_LR": [True, True], "NUM_AGENTS_PER_TYPE": [1, 1], "SEED": 2,
         "CUDA_GRAPHS": True, **{sw.key: False for sw in SWITCHES},
         "NUM_STEPS_EVAL": None}   # NUM_STEPS_EVAL None: NUM_STEPS
    c.update(kw)
    return c


def head_sizes(n):
    """``action_space.n`` as the network takes it: an int (Discrete), or the list of a MultiDiscrete
    space, a list of one collapsing to its int (:236-237)."""
    if isinstance(n, (list, tuple)):
        return int(n[0]) if len(n) == 1 else [int(x) for x in n]
    return n


class ActorCriticRNN(nn.Module):
    def __init__(self, obs_dim: int, n_actions: Union[int, Sequence[int]], fc: int, hidden: int):
        """n_actions: the size of a Discrete space, or the list of a MultiDiscrete one: then ``actor2``
        stacks one head per entry (``nvec``; rows off_k .. off_k + nvec[k] are head k), each
        initialised as the separate Dense layer it is in the reference.  A list of one is a
        single head (:236-237)."""
        super().__init__()
        n_actions = head_sizes(n_actions)
        self.nvec = n_actions if isinstance(n_actions, list) else None
        self.heads: List[int] = [n_actions] if self.nvec is None else self.nvec   # the heads' widths, one or more
        n_actions = sum(self.heads)
        self.embed = nn.Linear(obs_dim, fc)
        self.gru = nn.GRUCell(fc, hidden)
        self.critic1, self.critic2 = nn.Linear(hidden, fc), nn.Linear(fc, 1)
        self.actor1, self.actor2 = nn.Linear(hidden, hidden), nn.Linear(hidden, n_actions)
        for m, g in ((self.embed, math.sqrt(2)), (self.critic1, 2.0), (self.critic2, 1.0), (self.actor1, 2.0),
                     (self.actor2, 0.01)):
            nn.init.orthogonal_(m.weight, g)
            nn.init.zeros_(m.bias)
        if len(self.heads) > 1:   # (one head is the layer just initialised: no further draw from the generator)
            with torch.no_grad():
                for blk in self.actor2.weight.split(self.heads, 0):
                    blk.copy_(nn.init.orthogonal_(torch.empty_like(blk), 0.01))
        self.hidden = hidden
        self.fused = False   # forward's scan as one HIP launch per direction (train.gru.gru_scan); the trainer sets it
        # the narrow layers' weight and bias gradients through train.wgrad.narrow_linear; the trainer sets it
        self.fused_wgrad = False
        # the wide layers' (gru.weight_ih, actor1, critic1, and with ``fused`` gru.weight_hh) weight and bias
        # gradients through train.wgrad.wide_linear and train.gru.weight_grads_fused; the trainer sets it
        self.fused_wgrad_wide = False

    def _linear(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, wide: bool = False) -> torch.Tensor:
        """A layer of the sequence forward: ``F.linear`` (what a Linear module is on its own weight and bias),
        with the fused weight gradient behind it where the layer's flag is set: ``fused_wgrad`` for a narrow
        layer, ``fused_wgrad_wide`` for a wide one."""
        on, fused = (self.fused_wgrad_wide, wide_linear) if wide else (self.fused_wgrad, narrow_linear)
        return fused(x, w, b) if on else F.linear(x, w, b)

    def action_shape(self, *lead: int) -> tuple:
        """The shape of the public action tensor of ``lead`` actors: one word each for a Discrete space,
        K words for a MultiDiscrete one (the one place that tells the two apart)."""
        return lead if self.nvec is None else lead + (len(self.heads),)

    def step(self, h: torch.Tensor, obs: torch.Tensor, done: torch.Tensor):
        """One time step for a batch of actors: (new carry, logits, value)."""
        h = torch.where(done[:, None], torch.zeros_like(h), h)
        h = self.gru(F.relu(self.embed(obs)), h)
        v = self.critic2(F.relu(self.critic1(h))).squeeze(-1)
        return h, self.actor2(F.relu(self.actor1(h))), v

    @staticmethod
    def scan_loop(gi_all, h0, dones, w_hh, b_hh):
        """The ScannedRNN scan as a loop over T, one GEMM and the gate math per step: hseq [T, B, H]."""
        # unbind / chunk (not slicing): their backward concatenates the per-step grads once,
        # where a slice's backward would zero-fill and add a whole [T, B, 3H] grad per step
        h = h0
        hs = []
        for t, gi in enumerate(gi_all.unbind(0)):
            h = torch.where(dones[t][:, None], torch.zeros_like(h), h)
            ir, iz, i_n = gi.chunk(3, -1)
            hr, hz, hn = F.linear(h, w_hh, b_hh).chunk(3, -1)
            r = torch.sigmoid(ir + hr)
            z = torch.sigmoid(iz + hz)
            n = torch.tanh(i_n + r * hn)
            h = (1.0 - z) * n + z * h
            hs.append(h)
        return torch.stack(hs)

    def gi_all(self, obs: torch.Tensor) -> torch.Tensor:
        """The input side of ``forward``: the embedding and the GRU's input projection over all T at once,
        [T, B, 3H] in gate order (r, z, n)."""
        e = self._linear(obs, self.embed.weight, self.embed.bias)
        return self._linear(F.relu(e), self.gru.weight_ih, self.gru.bias_ih, wide=True)

    def head_outputs(self, hseq: torch.Tensor):
        """The heads of ``forward`` on the scan's hseq [T, B, H]: logits [T, B, A], values [T, B]."""
        a1 = self._linear(hseq, self.actor1.weight, self.actor1.bias, wide=True)
        c1 = self._linear(hseq, self.critic1.weight, self.critic1.bias, wide=True)
        return (self._linear(F.relu(a1), self.actor2.weight, self.actor2.bias),
                self._linear(F.relu(c1), self.critic2.weight, self.critic2.bias).squeeze(-1))

    def forward(self, h0: torch.Tensor, obs: torch.Tensor, dones: torch.Tensor):
        """A sequence [T, B, ...] from carry h0 (the ScannedRNN scan): logits [T, B, A], values [T, B].
        The same cell as ``step``; the input-side GEMMs (embedding, the GRU's input
        projection, both heads) run once over all T, only h @ W_hh stays in the scan: the loop
        of ``scan_loop``, or with ``fused`` set one HIP launch forward and one backward."""
        return self.forward_grouped([self], [h0], [obs], [dones])[0]

    @staticmethod
    def forward_grouped(nets, h0s, obss, dones):
        """``forward`` of several independent nets on their own sequences: a list of (logits, values), net
        k's what the net gives alone, bit for bit.  Unless every net is ``fused`` each net's scan is its
        ``scan_loop``.  With every net ``fused``, one net's scan is ``gru_scan`` and several nets' scans are
        one HIP launch forward and one backward for all of them (``gru_scan_grouped``; the nets share T and
        the hidden size, each has its own B)."""
        gis = [net.gi_all(obs) for net, obs in zip(nets, obss)]
        w_hhs, b_hhs = [net.gru.weight_hh for net in nets], [net.gru.bias_hh for net in nets]
        fused_wgrad = all(net.fused_wgrad_wide for net in nets)
        if not all(net.fused for net in nets):
            hseqs = [net.scan_loop(*xs) for net, *xs in zip(nets, gis, h0s, dones, w_hhs, b_hhs)]
        elif len(nets) == 1:
            hseqs = [gru_scan(gis[0], h0s[0], dones[0], w_hhs[0], b_hhs[0], fused_wgrad)]
        else:
            hseqs = gru_scan_grouped(gis, h0s, dones, w_hhs, b_hhs, fused_wgrad=fused_wgrad)
        return [net.head_outputs(hseq) for net, hseq in zip(nets, hseqs)]


@dataclass
class Rollout:
    """One agent type's trajectory buffers, [T, n_actors, ...] on the device."""
    obs: torch.Tensor
    done: torch.Tensor          # the actor's done entering the step (GRU reset)
    global_done: torch.Tensor   # dones["__all__"] of the env (GAE)
    action: torch.Tensor
    value: torch.Tensor
    reward: torch.Tensor
    log_prob: torch.Tensor


def calculate_gae(reward, value, global_done, last_val, gamma: float, lam: float):
    """_calculate_gae (:668-690): reverse scan; returns (advantages, targets)."""
    T = reward.shape[0]
    adv = torch.empty_like(reward)
    gae = torch.zeros_like(last_val)
    next_value = last_val
    for t in range(T - 1, -1, -1):
        nd = 1.0 - global_done[t].to(reward.dtype)
        delta = reward[t] + gamma * next_value * nd - value[t]
        gae = delta + gamma * lam * nd * gae
        adv[t] = gae
        next_value = value[t]
    return adv, adv + value


def _loss_tail(log_prob, entropy, values, rb_value, rb_log_prob, gae, targets, clip_eps: float, vf_coef: float,
               ent_coef: float):
    """_loss_fn (:718-765) from the new log-probabilities [T, B] and the entropies [T, B] of the policy."""
    v_clip = rb_value + (values - rb_value).clamp(-clip_eps, clip_eps)
    value_loss = 0.5 * torch.maximum((values - targets) ** 2, (v_clip - targets) ** 2).mean()
    logratio = log_prob - rb_log_prob
    ratio = torch.exp(logratio)
    gae = (gae - gae.mean()) / (gae.std(unbiased=False) + 1e-8)
    actor_loss = -torch.minimum(ratio * gae, ratio.clamp(1.0 - clip_eps, 1.0 + clip_eps) * gae).mean()
    entropy = entropy.mean()
    approx_kl = ((ratio - 1) - logratio).mean()
    clip_frac = ((ratio - 1).abs() > clip_eps).float().mean()
    total = actor_loss + vf_coef * value_loss - ent_coef * entropy
    return total, value_loss, actor_loss, entropy, approx_kl, clip_frac


def ppo_loss_multi(logits, values, rb_action, rb_value, rb_log_prob, gae, targets, clip_eps: float, vf_coef: float,
                   ent_coef: float, nvec: Sequence[int]):
    """_loss_fn (:718-765) under MultiCategorical (:259-281) -> (total, value_loss, actor_loss, entropy,
    approx_kl, clip_frac): logits [..., sum(nvec)] are the heads' logits side by side, rb_action [..., K];
    log_prob is the sum of the heads' log-probabilities at their actions, entropy the sum of the heads'
    entropies, both starting from the first head's (one head adds nothing)."""
    log_prob = entropy = None
    for k, lg in enumerate(logits.split(list(nvec), dim=-1)):
        logp_all = F.log_softmax(lg, -1)
        lp = logp_all.gather(-1, rb_action[..., k].long().unsqueeze(-1)).squeeze(-1)
        ent = -(logp_all.exp() * logp_all).sum(-1)
        log_prob, entropy = (lp, ent) if k == 0 else (log_prob + lp, entropy + ent)
    return _loss_tail(log_prob, entropy, values, rb_value, rb_log_prob, gae, targets, clip_eps, vf_coef, ent_coef)


def ppo_loss(logits, values, rb_action, rb_value, rb_log_prob, gae, targets, clip_eps: float, vf_coef: float,
             ent_coef: float):
    """``ppo_loss_multi`` for a Discrete space: one head of all the logits, rb_action [...]."""
    return ppo_loss_multi(logits, values, rb_action[..., None], rb_value, rb_log_prob, gae, targets, clip_eps, vf_coef,
                          ent_coef, [logits.shape[-1]])


def linear_schedule(lr: float, count: int, n_minibatches: int, n_epochs: int, n_updates: int) -> float:
    """linear_schedule (:503-509): lr * (1 - (count // (minibatches * epochs)) / NUM_UPDATES)."""
    return lr * (1.0 - (count // (n_minibatches * n_epochs)) / n_updates)


def _average_grads(params, dist) -> None:
    """pmean of the gradients over ranks: one flattened all-reduce (bucket) per call."""
    grads = [p.grad for p in params if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat)
    flat /= dist.get_world_size()
    o = 0
    for g in grads:
        g.copy_(flat[o:o + g.numel()].view_as(g))
        o += g.numel()


def rollout_members(members: Sequence["IPPOTrainer"], env, state, tally: Optional[RolloutTally] = None):
    """NUM_STEPS of _env_step (:578-658) for the trainers ``members`` (one, or the several of a
    ``PopulationTrainer``) on one env batch whose rows [m E, (m + 1) E) are member m's; returns the env state.
    Per step: every member's policy side (with GROUPED_POLICY all the members' and types' steps as ONE launch),
    ONE ``env.step`` whose keys and per-type actions are the members' own concatenated, then every member's
    rows of the outputs into its buffers.  One member concatenates and slices nothing.
    With ``tally`` (TRAIN_DIAG: the accumulators of the whole env batch) the words of the update before are
    cleared at the top but for the running episode's, and every step's rewards, info record and global dones
    are folded in after its ``env.step``: one agents' tally and one world tally per step, on the same stream."""
    lead, P = members[0], len(members)
    E = lead.E
    if tally is not None:
        tally.begin()
    for t in range(lead.T):
        jobs: list = []
        actions = [m._policy_step(t, jobs) for m in members]
        if jobs:   # GROUPED_POLICY: the arguments of every policy_step_net the members would have launched
            nets, obss, dones, hs, keys, outs = zip(*jobs)
            policy_step_grouped(nets, obss, dones, hs, SAMPLE, keys=keys, outs=outs)
        keys = [m._next_keys() for m in members]
        if P == 1:
            keys, acts = keys[0], actions[0]
        else:
            keys, acts = torch.cat(keys), [torch.cat(a) for a in zip(*actions)]
        obs, state, rew, dones, _ = env.step(keys, state, acts, lead.params)
        if tally is not None:
            tally.step(env, dones)
        for k, m in enumerate(members):
            if P == 1:
                m._env_outputs(t, obs, rew, dones)
                continue
            r = slice(k * E, (k + 1) * E)
            m._env_outputs(t, [o[r] for o in obs], [x[r] for x in rew],
                           {"__all__": dones["__all__"][r], "agents": [d[r] for d in dones["agents"]]})
    return state


def run_rollout(owner, gens, rollout: Callable[[], None]) -> None:
    """``rollout()`` for ``owner`` (a trainer, or a population of them: its ``graphs``, ``_roll`` and
    ``_on_side_stream``): eager, or with CUDA_GRAPHS one eager rollout on a side stream (warm-up), then one
    capture (which runs nothing; ``gens`` are the torch generators it draws from), then replays.  A rollout that
    cannot be captured stays eager."""
    if not owner.graphs or owner._roll is False:
        return rollout()
    if owner._roll is None:  # one eager rollout (warm-up), then capture; capture runs nothing
        owner._on_side_stream(rollout)
        owner._roll = 0
        return None
    if owner._roll == 0:
        g = torch.cuda.CUDAGraph()
        for gen in gens:
            g.register_generator_state(gen)
        try:
            with torch.cuda.graph(g):
                rollout()
        except RuntimeError:  # an op that cannot be captured: stay eager
            owner._roll = False
            return rollout()
        owner._roll = g
    owner._roll.replay()
    return None


def joint_step(pairs) -> List[torch.Tensor]:
    """One PPO minibatch step of the (trainer, agent type) ``pairs`` from their static inputs: the forward over
    the sequences (``forward_grouped``: several nets' scans are grouped), each pair's loss with its trainer's
    coefficients, one backward, then per pair the grad pmean (multi-rank), the global-norm clip and Adam;
    returns each pair's loss scalars.  The pairs are one trainer's agent types, or with
    ``train.population.PopulationTrainer`` those of several trainers with the same switches."""
    T = pairs[0][0].T
    nets, bufs, sts = ([getattr(tr, x)[i] for tr, i in pairs] for x in ("nets", "buf", "_st"))
    idxs = [st["idx"] for st in sts]
    fw = ActorCriticRNN.forward_grouped(nets, [st["h0"][idx] for st, idx in zip(sts, idxs)],
                                        [b.obs[:, idx] for b, idx in zip(bufs, idxs)],
                                        [b.done[:, idx] for b, idx in zip(bufs, idxs)])
    outs = []
    for (tr, i), net, b, st, idx, (logits, values) in zip(pairs, nets, bufs, sts, idxs, fw):
        c = tr.c
        loss_fn = ppo_loss_fused if tr.fused_loss else ppo_loss_multi
        outs.append(loss_fn(logits, values, b.action[:, idx].view(T, -1, len(net.heads)), b.value[:, idx],
                            b.log_prob[:, idx], st["adv"][:, idx], st["tgt"][:, idx], c["CLIP_EPS"], c["VF_COEF"][i],
                            c["ENT_COEF"][i], net.heads))
    # the list of totals, not their sum: the grouped scan's backward runs once, when every net's
    # gradient of its hseq has arrived, and no net's gradient passes through an addition
    torch.autograd.backward([out[0] for out in outs])
    for (tr, i), net in zip(pairs, nets):
        if tr.dist is not None and tr.dist.get_world_size() > 1:
            _average_grads(list(net.parameters()), tr.dist)
        if tr.fused_opt:
            adam_clip_step(tr.opts[i], tr.c["MAX_GRAD_NORM"][i])
        else:
            torch.nn.utils.clip_grad_norm_(net.parameters(), tr.c["MAX_GRAD_NORM"][i])
            tr.opts[i].step()
    return [torch.stack([x.detach() for x in out]) for out in outs]


def run_joint_step(s: Dict, pairs, step: Callable[[], List[torch.Tensor]], graphs: bool, on_side_stream):
    """``step()``, a ``joint_step`` of ``pairs``, under the record ``s`` (warm, graph, out): eager, or with
    ``graphs`` two eager steps on a side stream, then one capture (which runs nothing), then replays."""
    if s["graph"] is None:
        for tr, i in pairs:
            tr.opts[i].zero_grad(set_to_none=True)
        if not graphs:
            return step()
        if s["warm"] < 2:
            r = on_side_stream(step)
            s["warm"] += 1
            return r
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s["out"] = step()
        s["graph"] = g
    s["graph"].replay()
    return [o.clone() for o in s["out"]]


class IPPOTrainer:
    """make_train(config)(rng) of the reference, one ``update`` per call."""

    def __init__(self, env: MARLEnv, config: Dict, dist=None, device=None, eval_env: Optional[MARLEnv] = None,
                 reset: bool = True):
        """reset=False leaves the env alone (``state`` stays None): the caller resets it with ``reset_keys`` and
        hands the first observations to ``_adopt_obs`` (``train.population``: one env batch for several trainers)."""
        self.env, self.c, self.dist, self.eval_env = env, config, dist, eval_env
        self.device = torch.device(device or env.device)
        nt = len(env.list_of_agents_configs)
        self.n_types = nt
        c = config
        for k in ("LR", "GAMMA", "GAE_LAMBDA", "ENT_COEF", "VF_COEF", "MAX_GRAD_NORM", "ANNEAL_LR"):
            c[k] = _per_type(c[k], nt)
        # NUM_ENVS is global, as in the reference's pmap learner: each of the N ranks steps
        # NUM_ENVS // N envs, NUM_UPDATES = TOTAL_TIMESTEPS // NUM_STEPS // NUM_ENVS
        # (ippo_rnn_JAXMARL_pmap.py:209-211, 329-332, 419)
        world = dist.get_world_size() if dist is not None else 1
        rank = dist.get_rank() if dist is not None else 0
        n_global = int(c["NUM_ENVS"])
        if n_global % world:
            raise ValueError(f"NUM_ENVS ({n_global}) must be a multiple of the world size ({world})")
        # GROUPED_SCAN: the agent types' minibatch steps in lockstep, their scans one launch per direction
        # (train.gru.gru_scan_grouped)
        if c.get("GROUPED_SCAN", False):
            if not c.get("FUSED_GRU", False):
                raise ValueError("GROUPED_SCAN needs FUSED_GRU")
            if nt > MAX_GROUPS:
                raise ValueError(f"GROUPED_SCAN needs <= {MAX_GROUPS} agent types, got {nt}")
            if world > 1:
                raise ValueError(f"GROUPED_SCAN is single-process (the gradient all-reduce is per agent type), "
                                 f"got a world size of {world}")
        # GROUPED_POLICY: the agent types' policy steps of a rollout step as one launch (train.policy.policy_step_grouped)
        if c.get("GROUPED_POLICY", False):
            if not c.get("FUSED_POLICY", False):
                raise ValueError("GROUPED_POLICY needs FUSED_POLICY")
            if nt > MAX_POLICY_GROUPS:
                raise ValueError(f"GROUPED_POLICY needs <= {MAX_POLICY_GROUPS} agent types, got {nt}")
        self.E, self.T = n_global // world, c["NUM_STEPS"]
        self.n_agents = list(env.multi_agent_config.number_of_agents_per_type)
        self.n_actors = [n * self.E for n in self.n_agents]
        self.num_updates = max(1, int(c["TOTAL_TIMESTEPS"] // self.T // n_global))
        for i, sp in enumerate(env.action_spaces):
            n = getattr(sp, "n", None)   # Dense(action_space.n): an int, or a MultiDiscrete space's list of ints
            if not isinstance(n, int) and not (isinstance(n, (list, tuple)) and n
                                               and all(isinstance(x, int) for x in n)):
                raise NotImplementedError(f"agent type {i}: IPPO-RNN needs a Discrete or MultiDiscrete action space "
                                          "(ippo_rnn_JAXMARL.py ActorCriticRNN)")
        torch.manual_seed(c["SEED"])  # the same initial parameters on every rank
        self.nets = [ActorCriticRNN(env.observation_spaces[i].shape[0], env.action_spaces[i].n, c["FC_DIM_SIZE"],
                                    c["GRU_HIDDEN_DIM"]).to(self.device) for i in range(nt)]
        # FUSED_GRU: the minibatch step's sequence scan through the fused operators (GPU only; off: the loop)
        if c.get("FUSED_GRU", False):
            if not gru_scan_supported(c["GRU_HIDDEN_DIM"]):
                raise ValueError(f"FUSED_GRU needs GRU_HIDDEN_DIM in {list(SUPPORTED_HIDDEN)}, "
                                 f"got {c['GRU_HIDDEN_DIM']}")
            for n in self.nets:
                n.fused = self.device.type == "cuda"
        # CALC_EVAL (:461-482, 876-975): after every update NUM_STEPS_EVAL sampled steps of the current nets
        # in a separate eval env, through the fused policy step and the tally launch (evaluate_policy)
        self.updates_done = 0
        if c.get("CALC_EVAL", False):
            self.T_eval = int(c.get("NUM_STEPS_EVAL") or self.T)
            if self.T_eval < 1:
                raise ValueError(f"NUM_STEPS_EVAL must be >= 1, got {self.T_eval}")
            if eval_env is None or not getattr(eval_env, "return_info", False):
                raise ValueError("CALC_EVAL needs eval_env, a second MARLEnv built with return_info=True")
        # TRAIN_DIAG: the rollout's steps tallied from the env's raw info record (train.diag)
        if c.get("TRAIN_DIAG", False) and not getattr(env, "return_info", False):
            raise ValueError('TRAIN_DIAG needs an env that writes the info record: build it with return_info="raw"')
        # every switch as the attribute of its name in lower case (fused_policy, fused_loss, fused_opt, grouped_scan,
        # fused_wgrad, fused_wgrad_wide, calc_eval, ...); one that is on passes its device and per-net checks
        for sw in SWITCHES:
            on = bool(c.get(sw.key, False))
            setattr(self, sw.key.lower(), on)
            if not on:
                continue
            if sw.gpu and self.device.type != "cuda":
                raise ValueError(f"{sw.key} needs a GPU device, got {self.device}")
            for i, n in enumerate(self.nets):
                err = sw.check(n, c) if sw.check else None
                if err:
                    raise ValueError(f"{err} (agent type {i})")
        for n in self.nets:   # the layers' weight gradients in the minibatch step (train.wgrad)
            n.fused_wgrad, n.fused_wgrad_wide = self.fused_wgrad, self.fused_wgrad_wide
        # the sets of agent types whose minibatch steps run as one: every type on its own, or all of them in lockstep
        groups = [list(range(nt))] if self.grouped_scan else [[i] for i in range(nt)]
        # HIP-graph minibatch steps: single process on the GPU (the grad all-reduce stays eager)
        self.graphs = bool(c.get("CUDA_GRAPHS", False)) and self.device.type == "cuda" and world == 1
        if self.graphs or self.fused_opt:  # capturable Adam: step counter and lr live on the device
            self.opts = [torch.optim.Adam(n.parameters(), lr=torch.tensor(c["LR"][i], device=self.device), eps=1e-5,
                                          capturable=True) for i, n in enumerate(self.nets)]
        else:
            self.opts = [torch.optim.Adam(n.parameters(), lr=c["LR"][i], eps=1e-5) for i, n in enumerate(self.nets)]
        if self.fused_opt:  # the state a first torch step would create, which the operator updates in place
            for opt in self.opts:
                init_adam_state(opt)
        self._roll = None        # the captured rollout graph (False: not capturable, stays eager)
        # one record per step group: its types, the eager steps run before the capture, the graph and its outputs
        self._steps = [{"types": g, "warm": 0, "graph": None, "out": None} for g in groups]
        self.opt_count = [0] * nt
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(c["SEED"] + 1000 * rank)
        self.params = env.default_params
        self._split = getattr(env, "split_keys", split_keys)   # device threefry split (jax.random.split)
        # rng = PRNGKey(SEED); rng, _rng = split(rng); reset keys = split(_rng, NUM_ENVS), sharded over
        # the ranks in order; each rank then draws its step keys from its own rng.  This follows the
        # SHAPE of the reference's key chain (:283-284, 329) but not its values: the reference also
        # splits rng once per agent type for the network init (:246) before the reset split, and
        # draws the per-device rngs as split(split(rng)[1], N_DEVICES) (:775-776).  The networks are
        # torch-initialised here, so the same SEED gives different reset / step keys than JAX.
        master = torch.tensor([[0, c["SEED"]]], dtype=torch.int32, device=self.device)
        k = self._split(master, 2)[0]
        self.rng = (k[0] if world == 1 else self._split(k[0:1].contiguous(), world)[0][rank]).clone()
        reset_keys = self._split(k[1:2].contiguous(), n_global)[0][rank * self.E:(rank + 1) * self.E].contiguous()
        self.reset_keys = reset_keys
        if self.fused_policy:
            # the sample keys' own chain, from a key no other chain uses (words "pol", SEED), so that
            # rng, the reset keys and every env step key are what they are without the switch
            pm = torch.tensor([[0x706F6C, c["SEED"]]], dtype=torch.int32, device=self.device)
            self.pol_rng = self._split(pm, world + 1)[0][rank + 1].clone()
        self.state = None
        if reset:
            obs, self.state = env.reset(reset_keys, self.params)
            self._adopt_obs(obs)
        self.last_done = [torch.zeros(n, dtype=torch.bool, device=self.device) for n in self.n_actors]
        self.h = [torch.zeros(n, c["GRU_HIDDEN_DIM"], device=self.device) for n in self.n_actors]
        T = self.T
        self.buf = [Rollout(obs=torch.empty((T, n, env.observation_spaces[i].shape[0]), device=self.device),
                            done=torch.empty((T, n), dtype=torch.bool, device=self.device),
                            global_done=torch.empty((T, n), dtype=torch.bool, device=self.device),
                            action=torch.empty(self.nets[i].action_shape(T, n), dtype=torch.int32, device=self.device),
                            value=torch.empty((T, n), device=self.device),
                            reward=torch.empty((T, n), device=self.device),
                            log_prob=torch.empty((T, n), device=self.device))
                    for i, n in enumerate(self.n_actors)]
        # the fixed-address inputs of each agent type's minibatch steps (what a captured graph reads)
        self._st = [{"h0": torch.empty((n, c["GRU_HIDDEN_DIM"]), device=self.device),
                     "adv": torch.empty((T, n), device=self.device),
                     "tgt": torch.empty((T, n), device=self.device),
                     "idx": torch.zeros(n // c["NUM_MINIBATCHES"], dtype=torch.long, device=self.device)}
                    for n in self.n_actors]
        # TRAIN_DIAG: the rollout's accumulators (a population's members share its tally: _diag_rows is then a
        # member's rows of it), each type's rollout_diag words and workspace, and the first minibatch step's scalars
        self._tally = RolloutTally(env, self.E, self.device) if self.train_diag and reset else None
        self._diag_rows = slice(0, self.E)
        if self.train_diag:
            self._diag_words = [torch.zeros(DIAG_WORDS, dtype=torch.float64, device=self.device)
                                for _ in self.n_actors]
            self._diag_ws = [torch.empty(max(1, diag_workspace(T * n)), dtype=torch.float64, device=self.device)
                             for n in self.n_actors]
        self._first = [None] * nt

    def _adopt_obs(self, obs) -> None:
        """The first observations after the reset, per agent type [E, n, D]."""
        self.last_obs = [o.reshape(n, -1).clone() for o, n in zip(obs, self.n_actors)]

    def _next_keys(self) -> torch.Tensor:
        """rng, _rng = split(rng); rng_step = split(_rng, NUM_ENVS) (:613-614)."""
        k = self._split(self.rng[None], 2)[0]
        self.rng.copy_(k[0])
        return self._split(k[1:2].contiguous(), self.E)[0].contiguous()

    @torch.no_grad()
    def rollout(self) -> None:
        """NUM_STEPS of _env_step (:578-658), all on the device; with CUDA_GRAPHS the whole
        rollout (policy, sampling, env steps, buffer writes) is one captured HIP graph."""
        return run_rollout(self, [self.gen], self._rollout)

    def _on_side_stream(self, fn):
        """fn() on a side stream between two joins with the current one: how eager work runs ahead of a capture."""
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            r = fn()
        torch.cuda.current_stream(self.device).wait_stream(side)
        return r

    def _rollout(self) -> None:
        self.state = rollout_members([self], self.env, self.state, self._tally)

    def _policy_step(self, t: int, jobs: list) -> list:
        """The policy side of rollout step t: per agent type the obs and done rows into the buffers, then the
        type's step, sample and log-prob.  Returns the env's view of the step's action words per type.  With
        GROUPED_POLICY the types' steps are not launched here but appended to ``jobs`` as the arguments of
        ``policy_step_net``, for the caller's one grouped launch; ``pol_rng`` is split per type in type order
        either way."""
        actions = []
        for i, net in enumerate(self.nets):
            b = self.buf[i]
            b.obs[t].copy_(self.last_obs[i])
            b.done[t].copy_(self.last_done[i])
            # the env's view of the step's action words: [E, n] for a Discrete type, [E, n, K] otherwise
            actions.append(b.action[t].view(net.action_shape(self.E, self.n_agents[i])))
            if self.fused_policy:  # pol_rng, sub = split(pol_rng); one launch: carry in place, outputs into the buffers
                k = self._split(self.pol_rng[None], 2)[0]
                self.pol_rng.copy_(k[0])
                job = (net, self.last_obs[i], self.last_done[i], self.h[i], k[1], (b.action[t], b.log_prob[t], b.value[t]))
                if self.grouped_policy:
                    jobs.append(job)
                else:
                    policy_step_net(*job[:4], SAMPLE, key=job[4], out=job[5])
                continue
            h, logits, v = net.step(self.h[i], self.last_obs[i], self.last_done[i])
            self.h[i].copy_(h)
            b.value[t].copy_(v)
            # one draw per head, in head order; log_prob adds the heads' from the first one's
            words = b.action[t].view(self.n_actors[i], len(net.heads))
            for k, lg in enumerate(logits.split(net.heads, -1)):
                a = torch.multinomial(torch.softmax(lg, -1), 1, generator=self.gen)
                words[:, k].copy_(a.squeeze(-1))
                lpk = torch.log_softmax(lg, -1).gather(-1, a).squeeze(-1)
                lp = lpk if k == 0 else lp + lpk
            b.log_prob[t].copy_(lp)
        return actions

    def _env_outputs(self, t: int, obs, rew, dones) -> None:
        """The env side of rollout step t: this trainer's rows of the step's outputs into its buffers."""
        for i in range(self.n_types):
            b = self.buf[i]
            b.reward[t].copy_(rew[i].reshape(-1))
            b.global_done[t].copy_(dones["__all__"].repeat_interleave(self.n_agents[i]))
            self.last_obs[i].copy_(obs[i].reshape(self.n_actors[i], -1))
            self.last_done[i].copy_(dones["agents"][i].reshape(-1))

    def _step(self, types: List[int]) -> List[torch.Tensor]:
        """One PPO minibatch step of the agent types ``types`` (``joint_step`` of this trainer's pairs)."""
        return joint_step([(self, i) for i in types])

    def _run_step(self, s: Dict) -> List[torch.Tensor]:
        """``_step`` of the step group with record ``s``, eager or captured (``run_joint_step``)."""
        types = s["types"]
        return run_joint_step(s, [(self, i) for i in types], lambda: self._step(types), self.graphs,
                              self._on_side_stream)

    def _prepare(self, i: int, h0: torch.Tensor) -> None:
        """After the rollout: agent type i's last value, GAE and the static inputs of its minibatch steps."""
        c, net, b, st = self.c, self.nets[i], self.buf[i], self._st[i]
        with torch.no_grad():
            _, _, last_val = net.step(self.h[i], self.last_obs[i], self.last_done[i])
            gae_fn = gae_fused if self.fused_loss else calculate_gae
            adv, targets = gae_fn(b.reward, b.value, b.global_done, last_val, c["GAMMA"][i], c["GAE_LAMBDA"][i])
            st["h0"].copy_(h0); st["adv"].copy_(adv); st["tgt"].copy_(targets)
            if self.train_diag:   # the type's rollout reduced to its diag words (eager, outside the graphs)
                if self.device.type == "cuda":
                    rollout_diag(b, st["adv"], st["tgt"], net.heads, out=self._diag_words[i], workspace=self._diag_ws[i])
                else:
                    self._diag_words[i].copy_(rollout_diag_reference(b, st["adv"], st["tgt"], net.heads))

    def _set_lr(self, i: int) -> None:
        """Agent type i's annealed learning rate for its next optimiser step, from its own ``opt_count``."""
        c = self.c
        if c["ANNEAL_LR"][i]:
            lr = linear_schedule(c["LR"][i], self.opt_count[i], c["NUM_MINIBATCHES"], c["UPDATE_EPOCHS"],
                                 self.num_updates)
            for g in self.opts[i].param_groups:
                if torch.is_tensor(g["lr"]):
                    g["lr"].fill_(lr)
                else:
                    g["lr"] = lr

    def update(self) -> Dict:
        """One _update_step: rollout, GAE, UPDATE_EPOCHS x NUM_MINIBATCHES PPO steps per agent type, one
        step group after the other (every type on its own, or with GROUPED_SCAN all the types in lockstep)."""
        c, mb = self.c, self.c["NUM_MINIBATCHES"]
        h0 = [h.clone() for h in self.h]
        self.rollout()
        for i in range(self.n_types):
            self._prepare(i, h0[i])
        perms = self._perms()
        stats = [torch.zeros(6, device=self.device) for _ in range(self.n_types)]
        for s in self._steps:
            for e in range(c["UPDATE_EPOCHS"]):
                for m in range(mb):
                    for i in s["types"]:
                        self._set_lr(i)
                        self._st[i]["idx"].copy_(perms[i][e][m])
                    for i, r in zip(s["types"], self._run_step(s)):
                        if e == 0 and m == 0:
                            self._first[i] = r
                        stats[i] += r
                        self.opt_count[i] += 1
        return self._metrics(stats)

    def _perms(self) -> List[List[torch.Tensor]]:
        """An update's permutations of the actors, [type][epoch] as [NUM_MINIBATCHES, n // NUM_MINIBATCHES]."""
        # every permutation up front, type 0's epochs, then type 1's, ...: the generator goes through one
        # sequence whatever the step groups are
        c, mb = self.c, self.c["NUM_MINIBATCHES"]
        return [[torch.randperm(n, device=self.device, generator=self.gen).view(mb, n // mb)
                 for _ in range(c["UPDATE_EPOCHS"])] for n in self.n_actors]

    def _metrics(self, stats: List[torch.Tensor]) -> Dict:
        """An update's metrics from each type's summed loss scalars; the update is counted."""
        c, mb = self.c, self.c["NUM_MINIBATCHES"]
        metrics = {"loss": [], "avg_reward": []}
        for i, b in enumerate(self.buf):
            stats[i] /= c["UPDATE_EPOCHS"] * mb
            metrics["loss"].append(dict(zip(("total_loss", "value_loss", "actor_loss", "entropy", "approx_kl",
                                             "clip_frac"), stats[i])))
            metrics["avg_reward"].append(b.reward.mean())
            if self.train_diag:   # the update's first minibatch step (epoch 0, minibatch 0): the reference's ratio_0 check
                metrics["loss"][i]["approx_kl_0"], metrics["loss"][i]["clip_frac_0"] = self._first[i][4], self._first[i][5]
        if self.train_diag:
            tally, rows = self._tally, self._diag_rows
            metrics["diag"] = TrainDiag(tally.stats[rows], tally.wstats[rows], self._diag_words, self.env.layout,
                                        [n.heads for n in self.nets], [n.nvec is not None for n in self.nets],
                                        self.env.type_names)
        if self.calc_eval:
            ev = self.evaluate(self.updates_done)
            metrics["eval"] = ev
            metrics["avg_reward_eval"] = [ev.reward(i)["mean"] for i in range(self.n_types)]
        self.updates_done += 1
        return metrics

    def eval_seed(self, update: int) -> int:
        """The seed of the evaluation after update number ``update`` (0 the first), from a key no other
        chain uses: word 0 of threefry2x32 under the key (words "evl", SEED) at the counter (rank,
        update), jax.random.fold_in's form.  Computed on the host: it reads no key the training carries."""
        import numpy as np
        from .policy import threefry2x32
        rank = self.dist.get_rank() if self.dist is not None else 0
        y0, _ = threefry2x32(0x65766C, int(self.c["SEED"]) & 0xFFFFFFFF, np.array([rank], np.uint32),
                             np.array([update & 0xFFFFFFFF], np.uint32))
        return int(y0[0])

    @torch.no_grad()
    def evaluate(self, update: int):
        """The reference's CALC_EVAL block (:943-975): a fresh reset of ``eval_env``, zero carries and
        NUM_STEPS_EVAL sampled steps of the current nets for this rank's envs, as
        ``evaluate_policy(eval_env, nets, E, NUM_STEPS_EVAL, eval_seed(update), greedy=False)``.  It runs
        eagerly, outside the captured graphs, and touches neither ``rng``, ``pol_rng`` nor torch's
        generator, so a run with CALC_EVAL trains bit for bit as one without."""
        from ..evaluate import evaluate_policy
        return evaluate_policy(self.eval_env, self.nets, self.E, self.T_eval, self.eval_seed(update), greedy=False)

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path: str) -> None:
        """torch.save of every net's state_dict, the optimisers' states, opt_count, the config and
        the env config (``env.config_name`` where the env carries one, else its dict)."""
        from dataclasses import asdict, is_dataclass
        mc = getattr(self.env, "multi_agent_config", None)
        env_cfg = getattr(self.env, "config_name", None) or (asdict(mc) if is_dataclass(mc) else None)
        torch.save({"format": CHECKPOINT_FORMAT, "nets": [n.state_dict() for n in self.nets],
                    "opts": [o.state_dict() for o in self.opts], "opt_count": list(self.opt_count),
                    "config": dict(self.c), "env_config": env_cfg,
                    "shapes": [(n.embed.in_features, head_sizes(n.heads)) for n in self.nets]}, path)

    def load_checkpoint(self, path: str) -> None:
        """Restores what ``save_checkpoint`` wrote into this trainer (same env and sizes).  The
        parameters are copied in place (a captured rollout stays valid); the optimisers get new
        state tensors, so the minibatch steps' graphs are captured again at the next update."""
        ck = _read_checkpoint(path)
        if len(ck["nets"]) != self.n_types:
            raise ValueError(f"{path}: {len(ck['nets'])} agent types, this trainer has {self.n_types}")
        capturable = self.graphs or self.fused_opt
        for net, opt, sd, od in zip(self.nets, self.opts, ck["nets"], ck["opts"]):
            net.load_state_dict(sd)
            for g in od["param_groups"]:   # capturable Adam keeps lr on the device, the eager one as a float
                g["capturable"] = capturable
                g["lr"] = torch.tensor(float(g["lr"]), device=self.device) if capturable else float(g["lr"])
            opt.load_state_dict(od)
            if self.fused_opt:   # (a checkpoint from before the first step carries no state)
                init_adam_state(opt)
        self.opt_count = list(ck["opt_count"])
        for s in self._steps:
            s.update(warm=0, graph=None, out=None)


CHECKPOINT_FORMAT = "hftlob-ippo-1"


def _read_checkpoint(path: str) -> Dict:
    # onto the CPU: load_state_dict copies into the parameters and moves the optimiser state itself
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or ck.get("format") != CHECKPOINT_FORMAT:
        raise ValueError(f"{path} is not an IPPOTrainer checkpoint ({CHECKPOINT_FORMAT})")
    return ck


def load_policy(path: str, env=None, device=None) -> List[ActorCriticRNN]:
    """The nets of a checkpoint alone (eval mode, on ``device``, default the env's), one per agent
    type; with ``env`` given their sizes are checked against its observation and action spaces."""
    device = torch.device(device or (env.device if env is not None else "cpu"))
    ck = _read_checkpoint(path)
    c = ck["config"]
    nets = []
    for i, (sd, (D, A)) in enumerate(zip(ck["nets"], ck["shapes"])):
        A = head_sizes(A)   # an int, or a multi-head net's nvec
        if env is not None and (env.observation_spaces[i].shape[0] != D or head_sizes(env.action_spaces[i].n) != A):
            raise ValueError(f"{path}: agent type {i} has obs {D} / {A} actions, the env "
                             f"{env.observation_spaces[i].shape[0]} / {env.action_spaces[i].n}")
        net = ActorCriticRNN(D, A, c["FC_DIM_SIZE"], c["GRU_HIDDEN_DIM"]).to(device)
        net.load_state_dict(sd)
        nets.append(net.eval())
    if env is not None and len(nets) != len(env.action_spaces):
        raise ValueError(f"{path}: {len(nets)} agent types, the env has {len(env.action_spaces)}")
    return nets


def train(env: MARLEnv, config: Dict, n_updates: Optional[int] = None, dist=None, log=print, eval_env=None):
    """Runs ``n_updates`` (default NUM_UPDATES) updates; returns (trainer, env-steps/s over the run, the
    CALC_EVAL steps in ``eval_env`` not counted)."""
    tr = IPPOTrainer(env, config, dist=dist, eval_env=eval_env)
    n = n_updates or tr.num_updates
    sync = torch.cuda.synchronize if tr.device.type == "cuda" else (lambda: None)
    sync()
    t0 = time.perf_counter()
    for u in range(n):
        m = tr.update()
        if log is not None:
            rec = {"update": u, "avg_reward": [float(r) for r in m["avg_reward"]],
                   "loss": [{k: float(v) for k, v in d.items()} for d in m["loss"]]}
            if "avg_reward_eval" in m:
                rec["avg_reward_eval"] = [float(r) for r in m["avg_reward_eval"]]
            if "diag" in m:
                rec["diag"] = m["diag"].summary()
            log(rec)
    sync()
    world = dist.get_world_size() if dist is not None else 1
    return tr, n * tr.T * tr.E * world / (time.perf_counter() - t0)   # E * world = NUM_ENVS


def main(argv=None) -> None:
    """python -m hftlob.train.ippo [--rl-config ippo.yaml] [--env-config 2_player_fq_fqc] [--updates N]
    [switch flags: one per row of SWITCHES, --fused-gru ... --calc-eval, --train-diag]
    [--seeds 2,3,4,5 [--overrides sweep.yaml]]: the runs of a sweep as one population (train.population)"""
    import argparse
    import json
    import yaml
    from ..config_io import builtin_config, load_config_from_file
    ap = argparse.ArgumentParser()
    ap.add_argument("--rl-config", default=None, help="reference-style YAML (ippo_rnn_JAXMARL_2player.yaml keys)")
    ap.add_argument("--env-config", default="2_player_fq_fqc", help="JSON path or builtin config name")
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--envs", type=int, default=None)
    for sw in SWITCHES:
        ap.add_argument(sw.flag, action="store_true", help=sw.help)
    ap.add_argument("--save", default=None, metavar="PATH", help="write a checkpoint here after the last update")
    ap.add_argument("--seeds", default=None, metavar="S0,S1,...", help="train one independent run per seed in lockstep "
                    "in this process (train.population.PopulationTrainer); --save PATH writes PATH.m0, PATH.m1, ...")
    ap.add_argument("--overrides", default=None, metavar="YAML", help="with --seeds: a YAML list of per-member dicts "
                    "over LR, GAMMA, GAE_LAMBDA, CLIP_EPS, ENT_COEF, VF_COEF, MAX_GRAD_NORM, ANNEAL_LR, TOTAL_TIMESTEPS, SEED")
    ap.add_argument("--data", default=None, help="'lobster' to load world_config.dataPath (else synthetic)")
    a = ap.parse_args(argv)
    c = default_config()
    if a.rl_config:
        with open(a.rl_config) as f:
            c.update({k: v for k, v in yaml.safe_load(f).items() if k in c})
    if a.envs:
        c["NUM_ENVS"] = a.envs
    for sw in SWITCHES:
        if getattr(a, sw.key.lower()):
            c[sw.key] = True
    cfg = (load_config_from_file(a.env_config) if a.env_config.endswith((".json", ".yaml"))
           else builtin_config(a.env_config))
    # TRAIN_DIAG reads the steps' raw info record; the info dict is never built
    env = MARLEnv(None, cfg, data=a.data, return_info="raw" if c["TRAIN_DIAG"] else False, persistent_outputs=True)
    if not a.env_config.endswith((".json", ".yaml")):
        env.config_name = a.env_config   # what a checkpoint records instead of the config's dict
    if a.overrides and not a.seeds:
        raise ValueError("--overrides needs --seeds")
    if a.seeds:
        from . import population as P
        seeds = P.parse_seeds(a.seeds)
        configs = P.member_configs(c, seeds, P.load_overrides(a.overrides, len(seeds)) if a.overrides else None)
        pop, sps = P.train_population(env, configs, a.updates, log=lambda m: print(json.dumps(m)))
        if a.save:
            for k, m in enumerate(pop.members):
                m.save_checkpoint(f"{a.save}.m{k}")
        print(json.dumps({"env_steps_per_s_incl_learner": sps, "members": len(seeds), "num_envs": c["NUM_ENVS"],
                          "num_steps": c["NUM_STEPS"]}))
        return
    eval_env = None
    if c["CALC_EVAL"]:
        from ..data.synthetic import generate_day
        w = cfg.world_config
        day = generate_day(seed=1, snap_every=w.n_data_msg_per_step * w.start_resolution)
        eval_env = MARLEnv(None, cfg, data=day, return_info=True, persistent_outputs=True)
    tr, sps = train(env, c, a.updates, log=lambda m: print(json.dumps(m)), eval_env=eval_env)
    if a.save:
        tr.save_checkpoint(a.save)
    print(json.dumps({"env_steps_per_s_incl_learner": sps, "num_envs": c["NUM_ENVS"], "num_steps": c["NUM_STEPS"]}))


if __name__ == "__main__":
    main()
