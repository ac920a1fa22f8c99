"""The update's GAE and PPO objective (_calculate_gae, ippo_rnn_JAXMARL.py:668-690; _loss_fn,
:718-765, under MultiCategorical, :259-281) as two engine operators and their autograd wrapper.

``gae_reference`` and ``ppo_loss_reference`` restate ``hftlob_gae`` and ``hftlob_ppo_loss``
(include/hftlob.h) in torch, in whatever float type they are given: they are the spec of the kernels
and what the tests compare against.  ``train.ippo.calculate_gae`` and ``train.ippo.ppo_loss_multi``
stay the definitions: ``gae_reference`` in float32 is ``calculate_gae`` bit for bit, and
``ppo_loss_reference`` is ``ppo_loss_multi`` with the closed form of what autograd makes of it.
``gae`` and ``ppo_loss_fused`` are the fused paths: one launch, and three launches that write the
gradient in the same pass as the loss.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from .. import _lib
from .policy import MAX_ACTIONS, MAX_HEADS

ROWS = 64        # HFTLOB_PPO_LOSS_ROWS: elements per workgroup of the element pass
_WS_HEAD, _WS_ROW = 128, 5   # HFTLOB_PPO_LOSS_WS_HEAD, HFTLOB_PPO_LOSS_WS_ROW


def workspace_doubles(N: int) -> int:
    """HFTLOB_PPO_LOSS_WORKSPACE(N): the doubles ``hftlob_ppo_loss`` needs for N elements."""
    return _WS_HEAD + _WS_ROW * ((int(N) + ROWS - 1) // ROWS)


def ppo_loss_supported(nvec: Sequence[int]) -> bool:
    """Whether the fused loss takes these head widths (no GPU needed to ask)."""
    nvec = list(nvec)
    return 1 <= len(nvec) <= MAX_HEADS and all(1 <= int(n) <= MAX_ACTIONS for n in nvec)


# ------------------------------------------------------------------ GAE
def _gae_scalars(gamma: float, lam: float):
    """(gamma, gamma * lambda) as the operator takes them: the product in double, both rounded to float32."""
    return C.c_float(float(gamma)).value, C.c_float(float(gamma) * float(lam)).value


def gae_reference(reward, value, done, last_val, gamma: float, lam: float):
    """hftlob_gae: (adv [T, n], targets [T, n]); every operation separately rounded in the tensors' type."""
    g, gl = _gae_scalars(gamma, lam)
    if reward.dtype == torch.float64:   # the spec in float64 keeps the scalars unrounded
        g, gl = float(gamma), float(gamma) * float(lam)
    adv, tgt = torch.empty_like(reward), torch.empty_like(reward)
    gae = torch.zeros_like(last_val)
    next_value = last_val
    for t in range(reward.shape[0] - 1, -1, -1):
        nd = 1.0 - done[t].to(reward.dtype)
        delta = (reward[t] + (g * next_value) * nd) - value[t]
        gae = delta + ((gl * nd) * gae)
        adv[t] = gae
        tgt[t] = gae + value[t]
        next_value = value[t]
    return adv, tgt


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _u8(done):
    done = done.detach().contiguous()
    return done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)


def gae(reward, value, done, last_val, gamma: float, lam: float):
    """hftlob_gae on device tensors [T, n]: (adv, targets), float32."""
    reward, value, last_val, done = _f32(reward), _f32(value), _f32(last_val), _u8(done)
    ptrs = [_lib.ptr(x) for x in (reward, value, done, last_val)]   # (a CPU tensor raises here)
    if reward.dim() != 2 or value.shape != reward.shape or done.shape != reward.shape \
            or last_val.shape != reward.shape[1:]:
        raise ValueError(f"gae: shapes reward {tuple(reward.shape)}, value {tuple(value.shape)}, done "
                         f"{tuple(done.shape)}, last_val {tuple(last_val.shape)} do not agree")
    T, n = reward.shape
    adv, tgt = torch.empty_like(reward), torch.empty_like(reward)
    g, gl = _gae_scalars(gamma, lam)
    _lib.check(_lib.lib().hftlob_gae(T, n, *ptrs, g, gl, _lib.ptr(adv), _lib.ptr(tgt),
                                     _lib.stream_ptr(device=reward.device)))
    return adv, tgt


# ------------------------------------------------------------------ the loss
def _flat(logits, values, actions, rb_value, rb_log_prob, adv, targets, nvec):
    nvec = [int(n) for n in nvec]
    S, K = sum(nvec), len(nvec)
    if logits.shape[-1] != S or actions.shape[-1] != K or logits.shape[:-1] != actions.shape[:-1]:
        raise ValueError(f"ppo_loss: logits {tuple(logits.shape)} and actions {tuple(actions.shape)} do not agree "
                         f"with the heads {nvec}")
    N = logits.numel() // S
    rest = [values, rb_value, rb_log_prob, adv, targets]
    if any(x.numel() != N for x in rest):
        raise ValueError(f"ppo_loss: {N} elements of logits, but values, rb_value, rb_log_prob, adv, targets have "
                         f"{[x.numel() for x in rest]}")
    return N, nvec, logits.reshape(N, S), actions.reshape(N, K), [x.reshape(N) for x in rest]


def ppo_loss_elements(logits, values, actions, rb_value, rb_log_prob, adv, targets, clip_eps: float,
                      nvec: Sequence[int]):
    """The per-element quantities of hftlob_ppo_loss over the flattened N elements, by the names of
    include/hftlob.h (A, ratio, lr, a, b, u, c, dv = v - rb_v, ent) and ``heads``, the (lp_k, p_k, H_k) of
    every head; ``terms`` are the five quantities whose means are the scalars before their factors:
    max(u^2, c^2), min(a, b), ent, (ratio - 1) - lr and [|ratio - 1| > eps]."""
    N, nvec, lg, act, (v, rbv, rblp, gae_, tgt) = _flat(logits, values, actions, rb_value, rb_log_prob, adv, targets,
                                                        nvec)
    eps = float(clip_eps)
    A = (gae_ - gae_.mean()) / (gae_.std(unbiased=False) + 1e-8)
    logp, ent, heads = 0.0, 0.0, []
    for k, x in enumerate(lg.split(nvec, -1)):
        lp = torch.log_softmax(x, -1)
        p = lp.exp()
        H = -(p * lp).sum(-1)
        logp = logp + lp.gather(-1, act[:, k].long().unsqueeze(-1)).squeeze(-1)
        ent = ent + H
        heads.append((lp, p, H))
    lr = logp - rblp
    ratio = lr.exp()
    a, b = ratio * A, ratio.clamp(1.0 - eps, 1.0 + eps) * A
    u, dv = v - tgt, v - rbv
    c = (rbv + dv.clamp(-eps, eps)) - tgt
    terms = (torch.maximum(u * u, c * c), torch.minimum(a, b), ent, (ratio - 1) - lr,
             ((ratio - 1).abs() > eps).to(lg.dtype))
    return dict(N=N, act=act, A=A, logp=logp, ent=ent, heads=heads, lr=lr, ratio=ratio, a=a, b=b, u=u, c=c, dv=dv,
                terms=terms)


def ppo_loss_reference(logits, values, actions, rb_value, rb_log_prob, adv, targets, clip_eps: float, vf_coef: float,
                       ent_coef: float, nvec: Sequence[int]):
    """hftlob_ppo_loss: ((total, value_loss, actor_loss, entropy, approx_kl, clip_frac), d_logits, d_values),
    the gradients of total in the shapes of logits and values.  Nothing here goes through autograd."""
    e = ppo_loss_elements(logits, values, actions, rb_value, rb_log_prob, adv, targets, clip_eps, nvec)
    eps, N = float(clip_eps), e["N"]
    A, ratio, a, b, u, c, dv = (e[k] for k in ("A", "ratio", "a", "b", "u", "c", "dv"))
    t = [x.mean() for x in e["terms"]]
    value_loss, actor_loss, entropy, approx_kl, clip_frac = 0.5 * t[0], -t[1], t[2], t[3], t[4]
    total = actor_loss + vf_coef * value_loss - ent_coef * entropy

    one = torch.ones_like(a)
    inside = ((ratio >= 1.0 - eps) & (ratio <= 1.0 + eps)).to(a.dtype)
    w = torch.where(a < b, one, torch.where(a > b, 0.0 * one, 0.5 + 0.5 * inside))
    g_lp = -A * w * ratio / N
    d_heads = []
    for k, (lp, p, H) in enumerate(e["heads"]):
        onehot = torch.zeros_like(p).scatter_(-1, e["act"][:, k].long().unsqueeze(-1), 1.0)
        d_heads.append(g_lp[:, None] * (onehot - p) + (ent_coef / N) * p * (lp + H[:, None]))
    vin = ((dv >= -eps) & (dv <= eps)).to(a.dtype)
    u2, c2 = u * u, c * c
    g_v = torch.where(u2 > c2, u, torch.where(u2 < c2, c * vin, 0.5 * u + 0.5 * c * vin))
    d_values = vf_coef * g_v / N
    return ((total, value_loss, actor_loss, entropy, approx_kl, clip_frac),
            torch.cat(d_heads, -1).reshape(logits.shape), d_values.reshape(values.shape))


def ppo_loss_op(logits, values, actions, rb_value, rb_log_prob, adv, targets, clip_eps: float, vf_coef: float,
                ent_coef: float, nvec: Sequence[int], grad: bool = True):
    """hftlob_ppo_loss on device tensors: (out6 [6], d_logits, d_values), the gradients ``None`` with
    ``grad`` off (the forward-only call).  The C entry point allocates nothing; this wrapper allocates
    the workspace, ``out6`` and the gradient tensors on every call (under a graph capture from the
    graph's pool).  Every action must lie in [0, nvec[k]): the operator does not check it."""
    N, nvec, lg, act, rest = _flat(logits, values, actions, rb_value, rb_log_prob, adv, targets, nvec)
    if not ppo_loss_supported(nvec):
        raise ValueError(f"ppo_loss: needs 1..{MAX_HEADS} heads of 1..{MAX_ACTIONS} actions, got {nvec}")
    lg, rest = _f32(lg), [_f32(x) for x in rest]
    act = act.detach().to(torch.int32).contiguous()
    v, rbv, rblp, gae_, tgt = rest
    ptrs = [_lib.ptr(x) for x in (lg, v, act, rbv, rblp, gae_, tgt)]   # (a CPU tensor raises here)
    dev = lg.device
    ws = torch.empty(workspace_doubles(N), dtype=torch.float64, device=dev)
    out6 = torch.empty(6, dtype=torch.float32, device=dev)
    d_logits = torch.empty(logits.shape, dtype=torch.float32, device=dev) if grad else None
    d_values = torch.empty(values.shape, dtype=torch.float32, device=dev) if grad else None
    _lib.check(_lib.lib().hftlob_ppo_loss(N, len(nvec), (C.c_int * len(nvec))(*nvec), *ptrs, float(clip_eps),
                                          float(vf_coef), float(ent_coef), _lib.ptr(ws), _lib.ptr(out6),
                                          _lib.ptr(d_logits), _lib.ptr(d_values), _lib.stream_ptr(device=dev)))
    return out6, d_logits, d_values


class PPOLoss(torch.autograd.Function):
    """out6 = hftlob_ppo_loss(...); element 0 is differentiable in logits and values (the stored
    gradients times the upstream gradient), the other five carry none."""

    @staticmethod
    def forward(ctx, logits, values, actions, rb_value, rb_log_prob, adv, targets, clip_eps, vf_coef, ent_coef, nvec):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out6, d_logits, d_values = ppo_loss_op(logits, values, actions, rb_value, rb_log_prob, adv, targets, clip_eps,
                                               vf_coef, ent_coef, nvec, grad=need)
        if need:
            ctx.save_for_backward(d_logits, d_values)
        return out6

    @staticmethod
    def backward(ctx, d_out):
        d_logits, d_values = ctx.saved_tensors
        g = d_out[0]    # (the other five elements are handed out detached: their upstream gradient is 0)
        return (d_logits * g, d_values * g) + (None,) * 9


def ppo_loss_fused(logits, values, rb_action, rb_value, rb_log_prob, gae, targets, clip_eps: float, vf_coef: float,
                   ent_coef: float, nvec: Sequence[int]):
    """``train.ippo.ppo_loss_multi`` through the fused operator: the same arguments ([T, B, ...] or
    flat) and the same 6-tuple; ``total`` is differentiable in logits and values, the rest detached."""
    out6 = PPOLoss.apply(logits, values, rb_action, rb_value, rb_log_prob, gae, targets, clip_eps, vf_coef, ent_coef,
                         nvec)
    return (out6[0],) + tuple(x.detach() for x in out6[1:].unbind(0))
