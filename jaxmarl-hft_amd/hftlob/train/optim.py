"""The update's optimiser step: ``torch.nn.utils.clip_grad_norm_`` followed by one step of
``torch.optim.Adam`` (Adam(eps 1e-5) after global-norm clipping, ippo_rnn_JAXMARL.py:524-533) as one
engine operator, ``hftlob_adam_clip`` (include/hftlob.h): two launches for all the tensors of a net.

``adam_clip_reference`` restates the operator in torch, in whatever float type it is given: it is the
spec of the kernel and what the tests compare against.  ``adam_clip_step`` is the fused step on an Adam
optimiser whose state ``init_adam_state`` created (or a torch step, or a checkpoint): the state stays
in the optimiser's own ``state`` dict, in capturable Adam's layout, and is updated in place, so
``state_dict()`` and the checkpoints are what they are without the operator.  The one difference from
the torch path: the gradients are read only, where ``clip_grad_norm_`` scales them in place.
"""
from __future__ import annotations

import math
from typing import Sequence

import torch

from .. import _lib

MAX_TENSORS = 16   # HFTLOB_ADAM_MAX_TENSORS
CHUNK = 1024       # HFTLOB_ADAM_CHUNK: elements per workgroup of the update pass
WORKSPACE = 64     # HFTLOB_ADAM_WORKSPACE: doubles


def adam_clip_supported(n_tensors: int) -> bool:
    """Whether the fused step takes a net of this many parameter tensors (no GPU needed to ask)."""
    return 1 <= int(n_tensors) <= MAX_TENSORS


def adam_clip_reference(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor],
                        exp_avgs: Sequence[torch.Tensor], exp_avg_sqs: Sequence[torch.Tensor], steps: Sequence,
                        lr, beta1: float, beta2: float, eps: float, max_norm: float):
    """hftlob_adam_clip: (params, exp_avgs, exp_avg_sqs, steps, total_norm) after the call, as new
    tensors (nothing given is modified).  The norm is summed in float64 and the scalars (coef, the bias
    corrections of every tensor's own step, the step size) are formed in float64 and rounded once to
    the tensors' type; the element math is in the tensors' type, every operation separately rounded."""
    dt = params[0].dtype
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    coef = max_norm / (total + 1e-6)
    coef = 1.0 if coef > 1.0 else coef               # (a NaN norm stays NaN)
    k = lambda x: torch.tensor(x, dtype=dt)          # noqa: E731  (the scalar rounded to the tensors' type)
    lr = float(lr)
    out_p, out_m, out_v, out_s = [], [], [], []
    for p, g, m, v, s in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
        st = float(s) + 1.0
        bc1, bc2 = 1.0 - beta1 ** st, 1.0 - beta2 ** st
        gc = g * k(coef)
        m = m + (gc - m) * k(1.0 - beta1)
        v = v * k(beta2) + k(1.0 - beta2) * (gc * gc)
        p = p - k(lr / bc1) * (m / (v.sqrt() / k(math.sqrt(bc2)) + k(eps)))
        out_p.append(p), out_m.append(m), out_v.append(v)
        out_s.append(torch.tensor(st, dtype=torch.float32))
    return out_p, out_m, out_v, out_s, k(total)


def init_adam_state(opt: torch.optim.Optimizer) -> None:
    """For every parameter of ``opt`` without state, what torch.optim.Adam(capturable=True) creates at
    its first step: ``step`` a float32 device scalar 0, ``exp_avg`` and ``exp_avg_sq`` zeros like the
    parameter."""
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state[p]
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def _f32c(t) -> bool:
    return torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous()


def adam_clip_step(opt: torch.optim.Adam, max_norm: float) -> torch.Tensor:
    """The fused clip_grad_norm_(params, max_norm) + opt.step() of an Adam optimiser of one param group
    (capturable, lr a float32 device tensor; no weight decay, amsgrad or maximize): parameters and
    state updated in place, the gradients left as they are.  Returns total_norm, a device scalar.  The
    workspace is allocated once per optimiser; the call itself is two launches on the current stream
    and can be captured in a HIP graph."""
    if not isinstance(opt, torch.optim.Adam) or len(opt.param_groups) != 1:
        raise ValueError("adam_clip_step: needs a torch.optim.Adam of one param group")
    group = opt.param_groups[0]
    if group.get("weight_decay", 0) or group.get("amsgrad", False) or group.get("maximize", False):
        raise ValueError("adam_clip_step: weight decay, amsgrad and maximize are not supported")
    params = group["params"]
    if not adam_clip_supported(len(params)):
        raise ValueError(f"adam_clip_step: needs 1..{MAX_TENSORS} parameter tensors, got {len(params)}")
    lr = group["lr"]
    if not (torch.is_tensor(lr) and lr.dtype == torch.float32 and lr.numel() == 1):
        raise ValueError("adam_clip_step: needs lr as a float32 device tensor (capturable Adam's)")
    rows = []
    for i, p in enumerate(params):
        st = opt.state[p]
        if len(st) == 0:
            raise ValueError(f"adam_clip_step: parameter {i} has no optimiser state (init_adam_state creates it)")
        g, m, v, step = p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"]
        if g is None:
            raise ValueError(f"adam_clip_step: parameter {i} has no .grad")
        if not (_f32c(p) and _f32c(g) and _f32c(m) and _f32c(v)):
            raise ValueError(f"adam_clip_step: parameter {i}, its .grad and its state must be float32 and contiguous")
        if not (_f32c(step) and step.numel() == 1) or g.numel() != p.numel() or m.numel() != p.numel() \
                or v.numel() != p.numel():
            raise ValueError(f"adam_clip_step: parameter {i}: step must be a float32 scalar tensor, .grad and the "
                             "state of the parameter's size")
        rows.append((p, g, m, v, step))
    ptr = _lib.ptr    # (a CPU tensor raises here)
    arr = (_lib.AdamTensor * len(rows))(*[_lib.AdamTensor(*[ptr(t) for t in r], r[0].numel()) for r in rows])
    dev = params[0].device
    ws = getattr(opt, "_adam_clip_workspace", None)
    if ws is None or ws.device != dev:
        ws = opt._adam_clip_workspace = torch.empty(WORKSPACE, dtype=torch.float64, device=dev)
    total_norm = torch.empty((), dtype=torch.float32, device=dev)
    beta1, beta2 = group["betas"]
    _lib.check(_lib.lib().hftlob_adam_clip(len(params), arr, _lib.ptr(lr), float(beta1), float(beta2),
                                           float(group["eps"]), float(max_norm), _lib.ptr(ws), _lib.ptr(total_norm),
                                           _lib.stream_ptr(device=dev)))
    return total_norm
