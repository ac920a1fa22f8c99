"""One ``ActorCriticRNN`` step for a batch of actors (ippo_rnn_JAXMARL.py:53-78, 183-256) with the
rollout's sample and log-probability, as one engine operator (``hftlob_policy_step``,
include/hftlob.h) and its restatement.

``policy_step_reference`` restates the operator in torch, in whatever float type it is given: it
is the spec of the kernel and what the tests compare against.  ``policy_step`` is the fused
path: one HIP launch, used by the trainer's rollout (``FUSED_POLICY``) and by
``hftlob.evaluate.evaluate_policy``.

``policy_step_multi`` and ``policy_step_multi_reference`` are the same pair for a MultiDiscrete
action space (``hftlob_policy_step_multi``): K categorical heads on the shared actor features
(MultiActionOutputIndependant / MultiCategorical, :80-100, 259-281), the rows of ``actor2`` stacked
head after head; head k samples with ``jax.random.split(key, K)[k]``, and one head is the
single-head operator with the key unsplit, as the reference collapses a list of one.  Both pairs
are one body over a list of head widths; ``policy_step_net`` steps an ``ActorCriticRNN`` through
the operator its heads need.  ``policy_step_grouped`` steps up to 8 independent nets, each as
``policy_step_net`` would, in one launch (``hftlob_policy_step_grouped``); its spec,
``policy_step_grouped_reference``, is the per-net reference in a loop.

Sampling (mode 0) is ``jax.random.categorical(key, logits)``: the first argmax of
``logits + g`` with ``g = jax.random.gumbel(key, (B, A))`` under the partitionable threefry
(``gumbel_noise``; the legacy threefry is not built).  Mode 1 is the first argmax of the logits.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np
import torch

from .. import _lib

SUPPORTED_HIDDEN = (64, 128, 256)   # GRU_HIDDEN_DIM and FC_DIM_SIZE of the kernel's instantiations (csrc/policy_step.hip)
MAX_OBS_DIM = 64
MAX_ACTIONS = 16                    # logits of one head: one 16-column MFMA block
MAX_HEADS = 4                       # heads of the multi-head operator (the price-level limit of fixed_prices)
SAMPLE, GREEDY = 0, 1               # the operator's modes

WEIGHT_NAMES = ("w_embed", "b_embed", "w_ih", "b_ih", "w_hh", "b_hh", "w_c1", "b_c1", "w_c2", "b_c2",
                "w_a1", "b_a1", "w_a2", "b_a2")


def policy_step_supported(D: int, FC: int, H: int, A: int) -> bool:
    """Whether the fused step has a kernel for these sizes (no GPU needed to ask)."""
    return (int(FC) in SUPPORTED_HIDDEN and int(H) in SUPPORTED_HIDDEN and 1 <= int(D) <= MAX_OBS_DIM
            and 1 <= int(A) <= MAX_ACTIONS)


def policy_step_multi_supported(D: int, FC: int, H: int, nvec: Sequence[int]) -> bool:
    """Whether the fused multi-head step has a kernel for these sizes (no GPU needed to ask)."""
    nvec = list(nvec)
    return (1 <= len(nvec) <= MAX_HEADS and all(policy_step_supported(D, FC, H, n) for n in nvec))


def net_weights(net) -> Dict[str, torch.Tensor]:
    """The parameters of an ``ActorCriticRNN`` under the names of ``hftlob_policy_weights`` (the
    parameters themselves, not copies); a dict of those names is returned as it is."""
    if isinstance(net, dict):
        return net
    return {"w_embed": net.embed.weight, "b_embed": net.embed.bias,
            "w_ih": net.gru.weight_ih, "b_ih": net.gru.bias_ih, "w_hh": net.gru.weight_hh, "b_hh": net.gru.bias_hh,
            "w_c1": net.critic1.weight, "b_c1": net.critic1.bias, "w_c2": net.critic2.weight, "b_c2": net.critic2.bias,
            "w_a1": net.actor1.weight, "b_a1": net.actor1.bias, "w_a2": net.actor2.weight, "b_a2": net.actor2.bias}


# ------------------------------------------------------------------ the noise, on the CPU
def threefry2x32(k0: int, k1: int, x0: np.ndarray, x1: np.ndarray):
    """threefry2x32 with 20 rounds on uint32 arrays of counters, as JAX runs it."""
    with np.errstate(over="ignore"):
        ks = [np.uint32(k0), np.uint32(k1), np.uint32(k0) ^ np.uint32(k1) ^ np.uint32(0x1BD11BDA)]
        x0 = (np.asarray(x0, dtype=np.uint32) + ks[0]).astype(np.uint32)
        x1 = (np.asarray(x1, dtype=np.uint32) + ks[1]).astype(np.uint32)
        rots = ((13, 15, 26, 6), (17, 29, 16, 24))
        for i in range(1, 6):
            for r in rots[(i - 1) % 2]:
                x0 = (x0 + x1).astype(np.uint32)
                x1 = ((x1 << np.uint32(r)) | (x1 >> np.uint32(32 - r))) ^ x0
            x0 = (x0 + ks[i % 3]).astype(np.uint32)
            x1 = (x1 + ks[(i + 1) % 3] + np.uint32(i)).astype(np.uint32)
    return x0, x1


def _key_words(key):
    if isinstance(key, torch.Tensor):
        key = key.detach().cpu().numpy()
    k = np.asarray(key).reshape(-1)
    if k.size != 2:
        raise ValueError("a key is two 32-bit words")
    return int(k[0]) & 0xFFFFFFFF, int(k[1]) & 0xFFFFFFFF


def random_bits(key, n: int) -> np.ndarray:
    """jax random_bits(key, 32, (n,)) under the partitionable threefry: uint32 [n], word i is
    y0 ^ y1 of threefry2x32(key, (0, i))."""
    k0, k1 = _key_words(key)
    y0, y1 = threefry2x32(k0, k1, np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    return y0 ^ y1


def gumbel_from_bits(bits) -> np.ndarray:
    """jax.random.gumbel's float32 draw from random words: f = bitcast((bits >> 9) | 0x3f800000) - 1,
    u = max(tiny, f (1 - tiny) + tiny), g = -log(-log(u)), all in float32."""
    bits = np.asarray(bits, dtype=np.uint32)
    tiny = np.finfo(np.float32).tiny
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    u = np.maximum(tiny, f * (np.float32(1.0) - tiny) + tiny).astype(np.float32)
    return (-np.log(-np.log(u))).astype(np.float32)


def split_key(key, n: int) -> np.ndarray:
    """jax.random.split(key, n) under the partitionable threefry, on the CPU: uint32 [n, 2], key j is
    (y0, y1) of threefry2x32(key, (0, j))."""
    k0, k1 = _key_words(key)
    y0, y1 = threefry2x32(k0, k1, np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    return np.stack([y0, y1], axis=1)


def head_keys(key, K: int) -> np.ndarray:
    """The heads' sample keys, uint32 [K, 2]: MultiCategorical.sample's split(key, K), and the key
    itself for one head (the reference builds a single categorical there and does not split)."""
    return split_key(key, K) if K > 1 else np.array([_key_words(key)], dtype=np.uint32)


def gumbel_noise(key, B: int, A: int) -> torch.Tensor:
    """jax.random.gumbel(key, (B, A)) under the partitionable threefry: float32 [B, A] on the CPU
    (element (b, a) is drawn from counter (0, b A + a))."""
    return torch.from_numpy(gumbel_from_bits(random_bits(key, B * A)).reshape(B, A))


# ------------------------------------------------------------------ the spec
def _trunk_reference(net_or_weights, obs, done, h):
    """Everything up to the logits, in the float type of ``obs``: (h [B, H], logits [B, S], value [B])."""
    dt, dev = obs.dtype, obs.device
    W = {k: v.detach().to(device=dev, dtype=dt) for k, v in net_weights(net_or_weights).items()}
    h = h.to(dt)
    hp = torch.where(done.bool()[:, None], torch.zeros_like(h), h)
    x = torch.relu(obs @ W["w_embed"].t() + W["b_embed"])
    ir, iz, i_n = (x @ W["w_ih"].t() + W["b_ih"]).chunk(3, -1)
    hr, hz, hn = (hp @ W["w_hh"].t() + W["b_hh"]).chunk(3, -1)
    r = torch.sigmoid(ir + hr)
    z = torch.sigmoid(iz + hz)
    n = torch.tanh(i_n + r * hn)
    hnew = (1.0 - z) * n + z * hp
    value = (torch.relu(hnew @ W["w_c1"].t() + W["b_c1"]) @ W["w_c2"].t() + W["b_c2"]).squeeze(-1)
    logits = torch.relu(hnew @ W["w_a1"].t() + W["b_a1"]) @ W["w_a2"].t() + W["b_a2"]
    return hnew, logits, value


def _head_reference(logits, gumbel):
    """One categorical head: the first argmax of logits (+ gumbel) and the log-softmax at it."""
    dev = logits.device
    score = logits if gumbel is None else logits + gumbel.to(device=dev, dtype=logits.dtype)
    # the first argmax: the smallest index among the maxima
    top = score.max(-1, keepdim=True).values
    A = logits.shape[-1]
    action = torch.where(score == top, torch.arange(A, device=dev), torch.full((), A, device=dev)).min(-1).values
    mx = logits.max(-1, keepdim=True).values
    logp = logits - mx - torch.log(torch.exp(logits - mx).sum(-1, keepdim=True))
    return action, logp.gather(-1, action[:, None]).squeeze(-1)


def policy_step_multi_reference(net_or_weights, obs, done, h, mode: int, nvec: Sequence[int], key=None, gumbel=None):
    """hftlob_policy_step_multi in torch, in the float type of ``obs`` (the weights are converted to
    it): returns (h [B, H], logits [B, S], value [B], action int64 [B, K], log_prob [B]).  Mode 0
    adds ``gumbel[k]`` [B, nvec[k]] to head k's logits, or ``gumbel_noise(head_keys(key, K)[k], B,
    nvec[k])``; log_prob adds the heads' log-probabilities in head order."""
    if mode not in (SAMPLE, GREEDY):
        raise ValueError("mode must be 0 (sample) or 1 (argmax)")
    nvec = [int(n) for n in nvec]
    hnew, logits, value = _trunk_reference(net_or_weights, obs, done, h)
    if logits.shape[1] != sum(nvec):
        raise ValueError(f"the actor head has {logits.shape[1]} rows, nvec {nvec} needs {sum(nvec)}")
    if mode == SAMPLE and gumbel is None:
        if key is None:
            raise ValueError("mode 0 needs key or gumbel")
        gumbel = [gumbel_noise(k, logits.shape[0], n) for k, n in zip(head_keys(key, len(nvec)), nvec)]
    actions, logp = [], None
    for k, lg in enumerate(logits.split(nvec, dim=-1)):
        a, lp = _head_reference(lg, gumbel[k] if mode == SAMPLE else None)
        actions.append(a)
        logp = lp if logp is None else logp + lp
    return hnew, logits, value, torch.stack(actions, -1), logp


def policy_step_reference(net_or_weights, obs, done, h, mode: int, key=None, gumbel=None):
    """hftlob_policy_step in torch: ``policy_step_multi_reference`` with the one head of all A rows of
    ``actor2`` (so the key is used unsplit), ``gumbel`` the head's [B, A] tensor, and the action
    int64 [B]."""
    A = net_weights(net_or_weights)["w_a2"].shape[0]
    hnew, logits, value, action, logp = policy_step_multi_reference(
        net_or_weights, obs, done, h, mode, [A], key=key, gumbel=None if gumbel is None else [gumbel])
    return hnew, logits, value, action.squeeze(-1), logp


# ------------------------------------------------------------------ the fused path
def _weights_struct(W: Dict[str, torch.Tensor], D: int, FC: int, H: int, A: int) -> _lib.PolicyWeights:
    shapes = {"w_embed": (FC, D), "b_embed": (FC,), "w_ih": (3 * H, FC), "b_ih": (3 * H,), "w_hh": (3 * H, H),
              "b_hh": (3 * H,), "w_c1": (FC, H), "b_c1": (FC,), "w_c2": (1, FC), "b_c2": (1,), "w_a1": (H, H),
              "b_a1": (H,), "w_a2": (A, H), "b_a2": (A,)}
    s = _lib.PolicyWeights()
    for name in WEIGHT_NAMES:
        t = W[name]
        if tuple(t.shape) != shapes[name] or t.dtype != torch.float32:
            raise ValueError(f"policy_step: {name} must be float32 {list(shapes[name])}, got {t.dtype} {list(t.shape)}")
        setattr(s, name, _lib.ptr(t.detach()))   # (a CPU or non-contiguous tensor raises here)
    return s


def _call_args(op: str, net, obs, done, h, mode: int, heads, flat: bool, key, out, h_out, logits: bool):
    """The operators' shared host side for one batch: shape checks, output allocation and the heads' keys,
    for the heads' widths ``heads`` over the rows of ``actor2``.  flat: the one head of hftlob_policy_step,
    whose action is [B]; else hftlob_policy_step_multi's [B, K].  Returns the sizes (B, D, FC, H, K, A),
    the weight struct and the tensors of the launch (obs, done, h, h_out, key or None, action, log_prob,
    value, logits or None)."""
    W = net_weights(net)
    if obs.dim() != 2 or h.dim() != 2:
        raise ValueError(f"{op}: obs must be [B, D] and h [B, H]")
    B, D = obs.shape
    H, K = h.shape[1], len(heads)
    FC, A = W["w_embed"].shape[0], W["w_a2"].shape[0]
    ashape = (B,) if flat else (B, K)
    if not policy_step_multi_supported(D, FC, H, heads) or sum(heads) != A:
        raise ValueError(f"{op} needs GRU_HIDDEN_DIM and FC_DIM_SIZE in {list(SUPPORTED_HIDDEN)}, an obs size "
                         f"in 1..{MAX_OBS_DIM} and 1..{MAX_HEADS} heads of 1..{MAX_ACTIONS} actions over the {A} rows "
                         f"of actor2, got H {H}, FC {FC}, D {D}, heads {heads}")
    if mode not in (SAMPLE, GREEDY):
        raise ValueError(f"{op}: mode must be 0 (sample) or 1 (argmax)")
    dev = obs.device
    if done.dtype == torch.bool:
        done = done.view(torch.uint8)
    h_out = h if h_out is None else h_out
    if out is None:
        out = (torch.empty(ashape, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.float32, device=dev))
    action, log_prob, value = out
    lg = torch.empty((B, A), dtype=torch.float32, device=dev) if logits else None
    for name, t, shape, dt in (("obs", obs, (B, D), torch.float32), ("done", done, (B,), torch.uint8),
                               ("h", h, (B, H), torch.float32), ("h_out", h_out, (B, H), torch.float32),
                               ("action", action, ashape, torch.int32), ("log_prob", log_prob, (B,), torch.float32),
                               ("value", value, (B,), torch.float32)):
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev:
            raise ValueError(f"{op}: {name} must be {dt} {list(shape)} on {dev}, got {t.dtype} "
                             f"{list(t.shape)} on {t.device}")
    if mode == SAMPLE:
        if key is None or key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2 or key.device != dev:
            raise ValueError(f"{op}: mode 0 needs key, a uint32/int32 tensor of 2 words on {dev}")
        if K > 1:   # head_keys on the device: [K, 2], one more small launch (one head takes the key unsplit)
            from ..env import split_keys
            key = split_keys(key.reshape(1, 2), K)[0]
    else:
        key = None
    return (B, D, FC, H, K, A), _weights_struct(W, D, FC, H, A), (obs, done, h, h_out, key, action, log_prob, value, lg)


def _fused_call(op: str, net, obs, done, h, mode: int, heads, flat: bool, key, out, h_out, logits: bool):
    """One batch through its operator: ``_call_args`` and the one launch."""
    (B, D, FC, H, K, A), ws, ts = _call_args(op, net, obs, done, h, mode, heads, flat, key, out, h_out, logits)
    obs, done, h, h_out, key, action, log_prob, value, lg = ts
    dev = obs.device
    args = (C.byref(ws), _lib.ptr(obs), _lib.ptr(done), _lib.ptr(h), _lib.ptr(h_out), int(mode), _lib.ptr(key),
            _lib.ptr(action), _lib.ptr(log_prob), _lib.ptr(value), _lib.ptr(lg), _lib.stream_ptr(device=dev))
    with torch.cuda.device(dev):
        if flat:
            rc = _lib.lib().hftlob_policy_step(B, D, FC, H, A, *args)
        else:
            rc = _lib.lib().hftlob_policy_step_multi(B, D, FC, H, K, (C.c_int * K)(*heads), *args)
        _lib.check(rc)
    return h_out, action, log_prob, value, lg


def policy_step(net, obs, done, h, mode: int, key=None, out=None, h_out=None, logits: bool = False):
    """hftlob_policy_step on device tensors: one launch on torch's current stream.

    net: an ``ActorCriticRNN`` (or a dict of its parameters by ``WEIGHT_NAMES``); the struct is
    built from the parameters' ``data_ptr()``s, which an in-place optimiser keeps valid across the
    replays of a captured graph.  obs float32 [B, D]; done bool / uint8 [B]; h float32 [B, H].
    mode 0 samples with ``key`` (uint32 / int32 [2] on the device), mode 1 takes the argmax.
    out: ``(action int32 [B], log_prob float32 [B], value float32 [B])`` to write into (for example
    rows of the rollout buffers); None allocates them.  h_out: where the new carry goes; None
    updates ``h`` in place.  Returns ``(h_out, action, log_prob, value, logits or None)``."""
    heads = [net_weights(net)["w_a2"].shape[0]]   # one head of all the rows of actor2
    return _fused_call("policy_step", net, obs, done, h, mode, heads, True, key, out, h_out, logits)


def policy_step_multi(net, obs, done, h, mode: int, nvec: Sequence[int], key=None, out=None, h_out=None,
                      logits: bool = False):
    """hftlob_policy_step_multi on device tensors: ``policy_step`` for a net whose ``actor2`` stacks
    the K heads of ``nvec``.  ``key`` is one key of 2 words, as for ``policy_step``: it is split
    into the heads' K keys on the device here (``split_keys``, one more small launch; nothing
    synchronises), and passed through for one head.  ``action`` is int32 [B, K], ``logits``
    [B, sum(nvec)]; the rest is as for ``policy_step``."""
    return _fused_call("policy_step_multi", net, obs, done, h, mode, [int(n) for n in nvec], False, key, out, h_out,
                       logits)


def policy_step_net(net, obs, done, h, mode: int, key=None, out=None):
    """One step of an ``ActorCriticRNN`` through the operator its action space needs, the carry ``h``
    updated in place: ``policy_step`` for a Discrete space (action [B]), ``policy_step_multi`` over
    ``net.heads`` for a MultiDiscrete one (action [B, K]).  Returns what they return."""
    flat = net.action_shape() == ()
    return _fused_call("policy_step" if flat else "policy_step_multi", net, obs, done, h, mode, net.heads, flat, key,
                       out, None, False)


# ------------------------------------------------------------------ several nets in one launch
MAX_GROUPS = 8   # HFTLOB_POLICY_MAX_GROUPS: the nets of one hftlob_policy_step_grouped launch


def _net_heads(net, heads):
    """(the heads' widths, flat) of a group: ``heads`` as given (an int is the one flat head of
    hftlob_policy_step, a list the heads of hftlob_policy_step_multi), else what ``policy_step_net`` takes
    from the net."""
    if heads is None:
        if isinstance(net, dict):
            raise ValueError("a dict of weights carries no action space: give its heads")
        return list(net.heads), net.action_shape() == ()
    if isinstance(heads, int):
        return [heads], True
    return [int(n) for n in heads], False


def policy_step_grouped_supported(nets, heads=None) -> bool:
    """Whether one grouped launch can step these nets (no GPU needed to ask): 1..8 of them, one
    FC_DIM_SIZE and one GRU_HIDDEN_DIM among them, and each one within the single operators' sizes."""
    nets = list(nets)
    if not 1 <= len(nets) <= MAX_GROUPS:
        return False
    Ws = [net_weights(n) for n in nets]
    FC, H = Ws[0]["w_embed"].shape[0], Ws[0]["w_hh"].shape[1]
    heads = [None] * len(nets) if heads is None else list(heads)
    return all(W["w_embed"].shape[0] == FC and W["w_hh"].shape[1] == H
               and policy_step_multi_supported(W["w_embed"].shape[1], FC, H, _net_heads(n, hd)[0])
               and sum(_net_heads(n, hd)[0]) == W["w_a2"].shape[0] for n, W, hd in zip(nets, Ws, heads))


def policy_step_grouped_reference(nets, obss, dones, hs, mode: int, keys=None, heads=None):
    """hftlob_policy_step_grouped in torch: the per-group reference in a loop.  A list of
    (h, logits, value, action, log_prob) as ``policy_step_multi_reference`` returns them, the action of a
    flat one-head group [B] as ``policy_step_reference``'s."""
    out = []
    for g, (net, obs, done, h) in enumerate(zip(nets, obss, dones, hs)):
        hd, flat = _net_heads(net, None if heads is None else heads[g])
        r = policy_step_multi_reference(net, obs, done, h, mode, hd, key=None if keys is None else keys[g])
        out.append(r[:3] + (r[3].squeeze(-1),) + r[4:] if flat else r)
    return out


def policy_step_grouped(nets, obss, dones, hs, mode: int, keys=None, outs=None, heads=None, h_outs=None,
                        logits: bool = False):
    """hftlob_policy_step_grouped on device tensors: one launch on torch's current stream that steps
    every net of ``nets`` (at most 8, of one FC_DIM_SIZE and GRU_HIDDEN_DIM) on its own batch.  Group g
    is what ``policy_step_net(nets[g], obss[g], dones[g], hs[g], mode, keys[g], outs[g])`` is, bit for
    bit: the same operator for the net's action space, the same split of the key into the heads' keys
    (one small launch per multi-head group in mode 0; nothing synchronises), the carry updated in place.
    ``heads`` (per group an int, a list, or None for the net's own), ``h_outs`` and ``logits`` are what
    ``policy_step`` / ``policy_step_multi`` take.  Returns a list of
    ``(h_out, action, log_prob, value, logits or None)``."""
    nets = list(nets)
    G = len(nets)
    op = "policy_step_grouped"
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"{op} takes 1..{MAX_GROUPS} nets, got {G}")
    if not len(obss) == len(dones) == len(hs) == G:
        raise ValueError(f"{op}: obss, dones and hs must have one entry per net")
    opt = lambda xs: [None] * G if xs is None else list(xs)  # noqa: E731
    keys, outs, heads, h_outs = opt(keys), opt(outs), opt(heads), opt(h_outs)
    groups = (_lib.PolicyGroup * G)()
    keep, res = [], []
    FC = H = dev = None
    for g, net in enumerate(nets):
        hd, flat = _net_heads(net, heads[g])
        (B, D, fc, hh, K, A), ws, ts = _call_args(f"{op}: group {g}", net, obss[g], dones[g], hs[g], mode, hd, flat,
                                                  keys[g], outs[g], h_outs[g], logits)
        if g == 0:
            FC, H, dev = fc, hh, ts[0].device
        elif (fc, hh) != (FC, H) or ts[0].device != dev:
            raise ValueError(f"{op}: the groups share FC_DIM_SIZE, GRU_HIDDEN_DIM and the device; group 0 has "
                             f"{FC}, {H} on {dev}, group {g} {fc}, {hh} on {ts[0].device}")
        x = groups[g]
        x.B, x.D, x.K, x.w = B, D, K, ws
        for k, n in enumerate(hd):
            x.nvec[k] = n
        for name, t in zip(("obs", "done", "h_in", "h_out", "keys", "action", "log_prob", "value", "logits"), ts):
            setattr(x, name, _lib.ptr(t))
        keep.append(ts)   # (the split keys live until the launch is queued)
        res.append((ts[3], ts[5], ts[6], ts[7], ts[8]))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hftlob_policy_step_grouped(FC, H, G, groups, int(mode), _lib.stream_ptr(device=dev)))
    return res
