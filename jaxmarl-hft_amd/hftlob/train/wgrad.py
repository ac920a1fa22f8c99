"""The weight and bias gradients of the net's narrow layers (``embed``: few inputs; ``actor2``, ``critic2``:
few outputs) as one engine operator, ``hftlob_xty`` (include/hftlob.h): a product reduced over all the
rows of the minibatch into an output of a few KB, split over the rows in two launches, where rocBLAS runs
the same GEMM on a handful of workgroups.

``xty_reference`` restates the operator in torch, in whatever float type it is given: it is the spec of
the kernel and what the tests compare against.  ``xty`` is the operator on device tensors.
``narrow_linear`` is ``F.linear`` with the operator behind its weight and bias gradients: the forward and
the data gradient stay torch's (rocBLAS), bit for bit.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from .. import _lib

STRIPE_ROWS = 128    # HFTLOB_XTY_STRIPE_ROWS
MAX_STRIPES = 512    # HFTLOB_XTY_MAX_STRIPES
MAX_P = 64           # HFTLOB_XTY_MAX_P: the narrow side
SUPPORTED_Q = (64, 128, 256)   # the wide side


def stripe_rule(N: int) -> Tuple[int, int]:
    """(G, rows) of hftlob_xty's stripe rule: G stripes of ``rows`` rows (the last one may be shorter), from
    N alone.  Up to MAX_STRIPES stripes of STRIPE_ROWS rows; past that the stripes grow, not their number."""
    N = int(N)
    if N <= 0:
        return 0, STRIPE_ROWS
    rows = STRIPE_ROWS if -(-N // STRIPE_ROWS) <= MAX_STRIPES else -(-N // MAX_STRIPES)
    return -(-N // rows), rows


def workspace_floats(N: int, P: int, Q: int) -> int:
    """What hftlob_xty_workspace documents: per stripe the partial C, sum_a and sum_b."""
    return stripe_rule(N)[0] * (P * Q + P + Q)


def narrow_linear_supported(in_features: int, out_features: int) -> bool:
    """Whether ``narrow_linear`` takes a layer of these sizes (no GPU needed to ask): one side in
    1..MAX_P, the other in SUPPORTED_Q."""
    i, o = int(in_features), int(out_features)
    return (1 <= o <= MAX_P and i in SUPPORTED_Q) or (1 <= i <= MAX_P and o in SUPPORTED_Q)


def xty_reference(A: torch.Tensor, B: torch.Tensor):
    """hftlob_xty: (C [P, Q], sum_a [P], sum_b [Q]) of A [N, P] and B [N, Q], in their own type."""
    return A.t() @ B, A.sum(0), B.sum(0)


def xty(A: torch.Tensor, B: torch.Tensor, want_sum_a: bool = False, want_sum_b: bool = False):
    """(C, sum_a, sum_b) of device tensors A [N, P] and B [N, Q] (float32, contiguous), the sums None
    unless asked for.  Two launches on the current stream; the outputs and the workspace are fresh
    ``torch.empty`` tensors, so the call can sit inside a ``torch.cuda.graph`` capture."""
    if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[0]:
        raise ValueError(f"xty: needs A [N, P] and B [N, Q], got {tuple(A.shape)} and {tuple(B.shape)}")
    if A.dtype != torch.float32 or B.dtype != torch.float32:
        raise ValueError("xty: needs float32 tensors")
    N, P = A.shape
    Q = B.shape[1]
    L = _lib.lib()
    n_ws = L.hftlob_xty_workspace(N, P, Q)
    if n_ws < 0:
        _lib.check(n_ws)
    pa, pb = _lib.ptr(A), _lib.ptr(B)   # (a CPU or non-contiguous tensor raises here)
    dev = A.device
    C = torch.empty((P, Q), dtype=torch.float32, device=dev)
    sa = torch.empty(P, dtype=torch.float32, device=dev) if want_sum_a else None
    sb = torch.empty(Q, dtype=torch.float32, device=dev) if want_sum_b else None
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    _lib.check(L.hftlob_xty(N, P, Q, pa, pb, _lib.ptr(C), _lib.ptr(sa), _lib.ptr(sb), _lib.ptr(ws),
                            _lib.stream_ptr(device=dev)))
    return C, sa, sb


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[..., W] flattened to contiguous, 16-byte aligned rows [N, W]."""
    t = t.reshape(-1, t.shape[-1]).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class _NarrowLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, d_y):
        x, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        # torch's own data gradient of the layer: the rows folded to 2-D, one mm
        d_x = d_y.reshape(-1, d_y.shape[-1]).mm(w).view(x.shape) if need_x else None
        d_w = d_b = None
        if need_w or need_b:
            out_f, in_f = w.shape
            if 1 <= out_f <= MAX_P and in_f in SUPPORTED_Q:   # narrow output (and a layer narrow on both sides)
                d_w, d_b, _ = xty(_rows(d_y), _rows(x), want_sum_a=bool(need_b))
            else:                                             # narrow input
                C, _, d_b = xty(_rows(x), _rows(d_y), want_sum_b=bool(need_b))
                d_w = C.t().contiguous()
        return d_x, (d_w if need_w else None), (d_b if need_b else None)


def narrow_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, w, b)`` for a layer that ``narrow_linear_supported`` accepts: the same forward and
    data gradient (``d_y @ w``, only when x needs one), bit for bit; d_w and d_b from one ``xty`` call over
    the rows flattened to [N, .].  GPU only: there is no other path behind it."""
    if not narrow_linear_supported(w.shape[1], w.shape[0]):
        raise ValueError(f"narrow_linear: a layer of {w.shape[1]} -> {w.shape[0]} is not supported (one side in "
                         f"1..{MAX_P}, the other in {list(SUPPORTED_Q)})")
    return _NarrowLinear.apply(x, w, b)
