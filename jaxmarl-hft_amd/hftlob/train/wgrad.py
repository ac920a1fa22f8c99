"""The weight and bias gradients of the net's narrow layers (``embed``: few inputs; ``actor2``, ``critic2``:
few outputs) as one engine operator, ``hftlob_xty`` (include/hftlob.h): a product reduced over all the
rows of the minibatch into an output of a few KB, split over the rows in two launches, where rocBLAS runs
the same GEMM on a handful of workgroups.

``xty_reference`` restates the operator in torch, in whatever float type it is given: it is the spec of
the kernel and what the tests compare against.  ``xty`` is the operator on device tensors.
``narrow_linear`` is ``F.linear`` with the operator behind its weight and bias gradients: the forward and
the data gradient stay torch's (rocBLAS), bit for bit.

The wide layers (``gru.weight_ih``, ``gru.weight_hh``, ``actor1``, ``critic1``: 64 to 768 outputs) have the
same shape of problem with an output too large for a lane's registers: ``hftlob_xty_wide`` tiles it over
the matrix cores (float32 in, float32 out, the numerics of an fmaf chain) and splits the rows by a rule of
(N, P, Q).  ``xty_wide_reference`` is its spec, ``xty_wide`` the operator, ``wide_linear`` the layer.
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

WIDE_MAX_P = 768          # HFTLOB_XTY_WIDE_MAX_P: the outputs of a wide layer, a multiple of 64
WIDE_TILE_P = 128         # HFTLOB_XTY_WIDE_TILE_P: rows of C in a workgroup's tile
WIDE_CHUNK = 32           # HFTLOB_XTY_WIDE_CHUNK: rows of A and B in an LDS chunk
WIDE_STRIPE_ROWS = 256    # HFTLOB_XTY_WIDE_STRIPE_ROWS
WIDE_TARGET_WGS = 512     # HFTLOB_XTY_WIDE_TARGET_WGS


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


def aligned(t: torch.Tensor) -> torch.Tensor:
    """t itself if it starts 16-byte aligned, else a (contiguous) copy that does."""
    return t.clone(memory_format=torch.contiguous_format) if t.data_ptr() % 16 else t


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[..., W] flattened to contiguous, 16-byte aligned rows [N, W]."""
    return aligned(t.reshape(-1, t.shape[-1]).contiguous())


class _Linear(torch.autograd.Function):
    """``F.linear(x, w, b)`` whose weight and bias gradients are ``wgrad(d_y rows [N, out], x rows [N, in],
    need_b) -> (d_w [out, in], d_b or None)``; the forward and the data gradient are torch's own."""

    @staticmethod
    def forward(ctx, wgrad, x, w, b):
        ctx.wgrad = wgrad
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, d_y):
        x, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3]
        # torch's own data gradient of the layer: the rows folded to 2-D, one mm
        d_x = d_y.reshape(-1, d_y.shape[-1]).mm(w).view(x.shape) if need_x else None
        d_w = d_b = None
        if need_w or need_b:
            d_w, d_b = ctx.wgrad(_rows(d_y), _rows(x), bool(need_b))
        return None, d_x, (d_w if need_w else None), (d_b if need_b else None)


def _narrow_wgrad(d_y, x, need_b):
    """``_Linear``'s wgrad for a narrow layer: one ``xty`` call, the narrow side as its A."""
    if 1 <= d_y.shape[1] <= MAX_P and x.shape[1] in SUPPORTED_Q:   # narrow output (and a layer narrow on both sides)
        d_w, d_b, _ = xty(d_y, x, want_sum_a=need_b)
        return d_w, d_b
    C, _, d_b = xty(x, d_y, want_sum_b=need_b)                     # narrow input
    return C.t().contiguous(), d_b


def _wide_wgrad(d_y, x, need_b):
    """``_Linear``'s wgrad for a wide layer: one ``xty_wide`` call."""
    return xty_wide([d_y], x, want_sum_a=need_b)


def narrow_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, w, b)`` for a layer that ``narrow_linear_supported`` accepts: the same forward and
    data gradient (``d_y @ w``, only when x needs one), bit for bit; d_w and d_b from one ``xty`` call over
    the rows flattened to [N, .].  GPU only: there is no other path behind it."""
    if not narrow_linear_supported(w.shape[1], w.shape[0]):
        raise ValueError(f"narrow_linear: a layer of {w.shape[1]} -> {w.shape[0]} is not supported (one side in "
                         f"1..{MAX_P}, the other in {list(SUPPORTED_Q)})")
    return _Linear.apply(_narrow_wgrad, x, w, b)


# ------------------------------------------------------------------ the wide layers
def wide_max_stripes(P: int, Q: int) -> int:
    """M of hftlob_xty_wide's stripe rule: the stripes that, times the tiles of C (WIDE_TILE_P rows by 64
    columns for Q = 64 and 128 otherwise), reach WIDE_TARGET_WGS workgroups."""
    tiles = -(-int(P) // WIDE_TILE_P) * (int(Q) // (64 if int(Q) == 64 else 128))
    return -(-WIDE_TARGET_WGS // tiles)


def wide_stripe_rule(N: int, P: int, Q: int) -> Tuple[int, int]:
    """(G, rows) of hftlob_xty_wide's stripe rule, from (N, P, Q): up to ``wide_max_stripes(P, Q)`` stripes
    of WIDE_STRIPE_ROWS rows; past that the stripes grow, not their number."""
    N, M = int(N), wide_max_stripes(P, Q)
    if N <= 0:
        return 0, WIDE_STRIPE_ROWS
    rows = WIDE_STRIPE_ROWS if -(-N // WIDE_STRIPE_ROWS) <= M else -(-N // M)
    return -(-N // rows), rows


def wide_workspace_floats(N: int, P: int, Q: int) -> int:
    """What hftlob_xty_wide_workspace documents: per stripe the partial C and sum_a."""
    return wide_stripe_rule(N, P, Q)[0] * (P * Q + P)


def wide_linear_supported(in_features: int, out_features: int) -> bool:
    """Whether ``wide_linear`` takes a layer of these sizes (no GPU needed to ask): the inputs in
    SUPPORTED_Q, the outputs a multiple of 64 up to WIDE_MAX_P."""
    i, o = int(in_features), int(out_features)
    return i in SUPPORTED_Q and 64 <= o <= WIDE_MAX_P and o % 64 == 0


def xty_wide_reference(a_blocks, B: torch.Tensor, head: Optional[torch.Tensor] = None, shift: int = 0,
                       zero_row: Optional[torch.Tensor] = None):
    """hftlob_xty_wide: (C [P, Q], sum_a [P]) of A = the blocks [N, cols_i] side by side and the rows
    ``zero_row[n] ? 0 : (n < shift ? head[n] : B[n - shift])``, in their own type.  A ``head`` of None is
    zeros; rows N - shift .. of B and the masked rows' values are not used."""
    A = torch.cat(list(a_blocks), 1)
    N, shift = A.shape[0], int(shift)
    rows = B[:N - shift]
    if shift:
        h = head[:shift] if head is not None else torch.zeros((shift, B.shape[1]), dtype=B.dtype, device=B.device)
        rows = torch.cat([h, rows], 0)
    if zero_row is not None:
        rows = torch.where(zero_row.bool()[:N, None], torch.zeros_like(rows), rows)
    return A.t() @ rows, A.sum(0)


def xty_wide(a_blocks, B: torch.Tensor, head: Optional[torch.Tensor] = None, shift: int = 0,
             zero_row: Optional[torch.Tensor] = None, want_sum_a: bool = False):
    """(C, sum_a) of device tensors, sum_a None unless asked for: ``a_blocks`` one or two float32 [N, cols_i]
    views with unit column stride (a column slice of a wider contiguous tensor is taken as it is), B float32
    contiguous [>= N - shift, Q], head [>= shift, Q], zero_row N bytes or bools.  Two launches on the current
    stream; the outputs and the workspace are fresh ``torch.empty`` tensors, so the call can sit inside a
    ``torch.cuda.graph`` capture."""
    blocks = list(a_blocks)
    if not 1 <= len(blocks) <= 2 or any(a.dim() != 2 for a in blocks) or B.dim() != 2:
        raise ValueError("xty_wide: needs one or two blocks [N, cols] of A and B [N, Q]")
    N, shift = blocks[0].shape[0], int(shift)
    if any(a.shape[0] != N for a in blocks) or B.shape[0] < N - shift:
        raise ValueError(f"xty_wide: needs A's blocks [N, cols] and B [>= N - shift, Q], got "
                         f"{[tuple(a.shape) for a in blocks]}, {tuple(B.shape)} and shift {shift}")
    if any(t.dtype != torch.float32 for t in blocks + [B]) or (head is not None and head.dtype != torch.float32):
        raise ValueError("xty_wide: needs float32 tensors")
    if head is not None and (head.dim() != 2 or head.shape[1] != B.shape[1] or head.shape[0] < shift):
        raise ValueError(f"xty_wide: needs head [>= shift, Q], got {tuple(head.shape)}")
    if zero_row is not None:
        zero_row = zero_row.reshape(-1)
        zero_row = zero_row.view(torch.uint8) if zero_row.dtype == torch.bool else zero_row.to(torch.uint8)
        if zero_row.numel() < N:
            raise ValueError(f"xty_wide: needs {N} bytes of zero_row, got {zero_row.numel()}")
    for a in blocks:
        if not a.is_cuda:
            raise RuntimeError("hftlob kernels need device (HIP) tensors; got a CPU tensor")
        if N > 1 and a.shape[1] and a.stride(1) != 1:
            raise RuntimeError("xty_wide: A's blocks need a unit column stride")
    P, Q = sum(a.shape[1] for a in blocks), B.shape[1]
    L = _lib.lib()
    n_ws = L.hftlob_xty_wide_workspace(N, P, Q)
    if n_ws < 0:
        _lib.check(n_ws)
    dev = B.device
    args = []
    for a in blocks + [None] * (2 - len(blocks)):
        args += [None, 0, 0] if a is None else [a.data_ptr(), a.shape[1], a.stride(0) if N > 1 else a.shape[1]]
    C = torch.empty((P, Q), dtype=torch.float32, device=dev)
    sa = torch.empty(P, dtype=torch.float32, device=dev) if want_sum_a else None
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    _lib.check(L.hftlob_xty_wide(N, Q, *args, _lib.ptr(B), _lib.ptr(head), shift, _lib.ptr(zero_row), _lib.ptr(C),
                                 _lib.ptr(sa), _lib.ptr(ws), _lib.stream_ptr(device=dev)))
    return C, sa


def wide_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, w, b)`` for a layer that ``wide_linear_supported`` accepts: the same forward and data
    gradient (``d_y @ w``, only when x needs one), bit for bit; d_w and d_b from one ``xty_wide`` call over
    the rows flattened to [N, .].  GPU only: there is no other path behind it."""
    if not wide_linear_supported(w.shape[1], w.shape[0]):
        raise ValueError(f"wide_linear: a layer of {w.shape[1]} -> {w.shape[0]} is not supported (inputs in "
                         f"{list(SUPPORTED_Q)}, outputs a multiple of 64 up to {WIDE_MAX_P})")
    return _Linear.apply(_wide_wgrad, x, w, b)
