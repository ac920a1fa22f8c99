"""Several independent IPPO runs ("members": the runs of a seed or hyper-parameter sweep, the reference's
``wandb.agent(sweep_id, function=sweep_fun)`` over ``SWEEP_PARAMETERS``) of ONE env config, trained in lockstep
in one process on one GPU.

A run of a few thousand envs leaves most of the chip idle: the update's GRU scan and the rollout's policy step
launch one workgroup per 16 actors, and the env step fills a fraction of its slots.  The
members share what is launched, not what is computed:

* one env batch of P x NUM_ENVS envs, member m owning the rows [m E, (m + 1) E): one ``env.step`` per rollout
  step, its keys and actions the members' own, concatenated;
* with ``GROUPED_POLICY`` one policy-step launch per rollout step for all P x n_types nets;
* one joint minibatch step over all (member, agent type) pairs: with ``FUSED_GRU`` one scan launch per
  direction, each pair's loss, clip and Adam with its member's coefficients;
* with ``TRAIN_DIAG`` one agents' tally and one world tally per rollout step for the whole batch
  (``train.diag.RolloutTally``), each member's ``metrics["diag"]`` reading its own rows.

Envs, nets and optimisers are independent, so every member's parameters, optimiser states, buffers, generator
and metrics are bit for bit those of a solo ``IPPOTrainer(env, config_m)`` with the same switches, and a
member's checkpoint is a solo trainer's.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import torch

from .gru import MAX_GROUPS
from .ippo import IPPOTrainer, joint_step, rollout_members, run_joint_step, run_rollout
from .policy import MAX_GROUPS as MAX_POLICY_GROUPS

# what the members of a population may differ in; every other key of their configs must agree
MEMBER_KEYS = ("SEED", "LR", "GAMMA", "GAE_LAMBDA", "CLIP_EPS", "ENT_COEF", "VF_COEF", "MAX_GRAD_NORM", "ANNEAL_LR",
               "TOTAL_TIMESTEPS")
ENV_KEYS = ("ENV_CONFIG", "AGENT_CONFIGS")   # a config's own env config (the reference's AGENT_CONFIGS sweeps)


def check_configs(configs: Sequence[Dict], n_types: int, device_type: str, world: int = 1) -> None:
    """The rules of a population's configs; a ValueError names what breaks them."""
    if not configs:
        raise ValueError("a population needs at least one config")
    if world > 1:
        raise ValueError(f"a population is single-process, got a world size of {world}")
    lead = configs[0]
    for m, c in enumerate(configs):
        for k in ENV_KEYS:
            if c.get(k) != lead.get(k):
                raise ValueError(f"the members of a population share one env config: member {m}'s {k} differs from "
                                 "member 0's (members with different env configs are not supported)")
        if c.get("CALC_EVAL", False):
            raise ValueError(f"CALC_EVAL is not supported in a population (member {m})")
        for k in sorted(set(lead) | set(c)):
            if k not in MEMBER_KEYS and c.get(k) != lead.get(k):
                raise ValueError(f"the members of a population must agree on {k}: member {m} has {c.get(k)!r}, "
                                 f"member 0 {lead.get(k)!r}")
    n = len(configs) * n_types
    fused_gru = lead.get("FUSED_GRU", False) and device_type == "cuda"
    for on, key, limit in ((fused_gru, "FUSED_GRU", MAX_GROUPS),
                           (lead.get("GROUPED_POLICY", False), "GROUPED_POLICY", MAX_POLICY_GROUPS)):
        if on and n > limit:
            raise ValueError(f"with {key} a population has at most {limit} nets (members x agent types), got "
                             f"{len(configs)} x {n_types} = {n}")


class PopulationTrainer:
    """``P = len(configs)`` independent ``IPPOTrainer`` runs of one env config, one ``update`` of all per call.

    ``members[m]`` is member m's trainer: its nets, optimisers, buffers, ``gen``, ``opt_count`` and
    ``save_checkpoint`` / ``load_checkpoint`` are a solo trainer's.  The members do not step on their own: the
    population owns the env state and drives their rollout and minibatch steps."""

    def __init__(self, env, configs: Sequence[Dict], dist=None, device=None):
        world = dist.get_world_size() if dist is not None else 1
        self.env, self.device = env, torch.device(device or env.device)
        nt = len(env.list_of_agents_configs)
        check_configs(configs, nt, self.device.type, world)
        self.members: List[IPPOTrainer] = [IPPOTrainer(env, c, device=device, reset=False) for c in configs]
        lead = self.members[0]
        self.E, self.T, self.graphs = lead.E, lead.T, lead.graphs
        # one env batch: the members' own reset keys, concatenated; member m owns the rows [m E, (m + 1) E)
        obs, self.state = env.reset(torch.cat([m.reset_keys for m in self.members]), lead.params)
        for k, m in enumerate(self.members):
            m._adopt_obs([o[k * self.E:(k + 1) * self.E] for o in obs])
        self._roll = None    # the captured population rollout (False: not capturable, stays eager)
        self.pairs = [(m, i) for m in self.members for i in range(nt)]
        # the one joint step's record; every member holds it as its only step group, so that a member's
        # load_checkpoint (new optimiser state tensors) makes the joint step capture again
        self._joint = {"types": list(range(nt)), "warm": 0, "graph": None, "out": None}
        for m in self.members:
            m._steps = [self._joint]
        # TRAIN_DIAG: one tally of the whole env batch; member m's diag reads its rows [m E, (m + 1) E)
        self._tally = None
        if lead.train_diag:
            from .diag import RolloutTally
            self._tally = RolloutTally(env, len(self.members) * self.E, self.device)
            for k, m in enumerate(self.members):
                m._tally, m._diag_rows = self._tally, slice(k * self.E, (k + 1) * self.E)

    _on_side_stream = IPPOTrainer._on_side_stream

    def _rollout(self) -> None:
        self.state = rollout_members(self.members, self.env, self.state, self._tally)

    @torch.no_grad()
    def rollout(self) -> None:
        """NUM_STEPS rollout steps of every member on the one env batch; with CUDA_GRAPHS one captured graph."""
        return run_rollout(self, [m.gen for m in self.members], self._rollout)

    def update(self) -> List[Dict]:
        """One _update_step of every member: the population rollout, each member's GAE and permutations, then
        UPDATE_EPOCHS x NUM_MINIBATCHES joint minibatch steps over all (member, agent type) pairs.  Returns
        the members' metrics dicts."""
        lead, members = self.members[0], self.members
        c, mb = lead.c, lead.c["NUM_MINIBATCHES"]
        h0 = [[h.clone() for h in m.h] for m in members]
        self.rollout()
        for m, hs in zip(members, h0):
            for i in range(m.n_types):
                m._prepare(i, hs[i])
        perms = {id(m): m._perms() for m in members}   # each member's own generator, in a solo update's order
        stats = {(id(m), i): torch.zeros(6, device=self.device) for m, i in self.pairs}
        for e in range(c["UPDATE_EPOCHS"]):
            for k in range(mb):
                for m, i in self.pairs:
                    m._set_lr(i)
                    m._st[i]["idx"].copy_(perms[id(m)][i][e][k])
                rs = run_joint_step(self._joint, self.pairs, lambda: joint_step(self.pairs), self.graphs,
                                    self._on_side_stream)
                for (m, i), r in zip(self.pairs, rs):
                    if e == 0 and k == 0:
                        m._first[i] = r
                    stats[id(m), i] += r
                    m.opt_count[i] += 1
        return [m._metrics([stats[id(m), i] for i in range(m.n_types)]) for m in members]


# ------------------------------------------------------------------ the command line's side
def parse_seeds(text: str) -> List[int]:
    """``--seeds 2,3,4,5`` -> [2, 3, 4, 5]."""
    try:
        seeds = [int(x) for x in text.split(",") if x.strip()]
    except ValueError:
        raise ValueError(f"--seeds takes a comma-separated list of integers, got {text!r}") from None
    if not seeds:
        raise ValueError("--seeds needs at least one seed")
    return seeds


def load_overrides(path: str, P: int) -> List[Dict]:
    """``--overrides sweep.yaml``: a YAML list of P per-member dicts over ``MEMBER_KEYS``."""
    import yaml
    with open(path) as f:
        ov = yaml.safe_load(f)
    if not isinstance(ov, list) or not all(isinstance(d, dict) for d in ov):
        raise ValueError(f"{path}: the overrides are a YAML list of per-member dicts")
    if len(ov) != P:
        raise ValueError(f"{path}: {len(ov)} override dicts for {P} members")
    for m, d in enumerate(ov):
        for k in d:
            if k not in MEMBER_KEYS:
                raise ValueError(f"{path}: member {m} overrides {k}; the members may differ in {', '.join(MEMBER_KEYS)}")
    return ov


def member_configs(base: Dict, seeds: Sequence[int], overrides: Optional[Sequence[Dict]] = None) -> List[Dict]:
    """One config per seed: a copy of ``base`` with the seed, then the member's overrides (which may set SEED too)."""
    overrides = [{}] * len(seeds) if overrides is None else overrides
    if len(overrides) != len(seeds):
        raise ValueError(f"{len(overrides)} override dicts for {len(seeds)} members")
    out = []
    for seed, ov in zip(seeds, overrides):
        c = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        c["SEED"] = int(seed)
        c.update(ov)
        out.append(c)
    return out


def train_population(env, configs: Sequence[Dict], n_updates: Optional[int] = None, log=print):
    """Runs ``n_updates`` (default the smallest NUM_UPDATES of the members) updates; logs one record per member
    and update; returns (population, aggregate env-steps/s over the run: all the members' envs)."""
    pop = PopulationTrainer(env, configs)
    n = n_updates or min(m.num_updates for m in pop.members)
    sync = torch.cuda.synchronize if pop.device.type == "cuda" else (lambda: None)
    sync()
    t0 = time.perf_counter()
    for u in range(n):
        for k, m in enumerate(pop.update()):
            if log is not None:
                rec = {"member": k, "seed": pop.members[k].c["SEED"], "update": u,
                       "avg_reward": [float(r) for r in m["avg_reward"]],
                       "loss": [{name: float(v) for name, v in d.items()} for d in m["loss"]]}
                if "diag" in m:
                    rec["diag"] = m["diag"].summary()
                log(rec)
    sync()
    return pop, n * pop.T * pop.E * len(pop.members) / (time.perf_counter() - t0)


__all__ = ["PopulationTrainer", "MEMBER_KEYS", "check_configs", "parse_seeds", "load_overrides", "member_configs",
           "train_population"]
