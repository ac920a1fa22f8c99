"""The learner's GRU sequence scan (ScannedRNN, ippo_rnn_JAXMARL.py:53-78) as two engine
operators and their autograd wrapper.

``gru_scan_grouped`` is the same scan for several independent nets at once (IPPO's one net per agent
type): ``hftlob_gru_scan_fwd_grouped`` / ``_bwd_grouped``, one launch per direction for all the groups,
every group's results bit for bit those of ``gru_scan`` on that group alone.

``gru_scan_reference`` / ``gru_scan_backward_reference`` restate ``hftlob_gru_scan_fwd`` /
``hftlob_gru_scan_bwd`` (include/hftlob.h) in torch, in whatever float type they are given: they
are the spec of the kernels and what the tests compare against.  ``gru_scan`` is the fused path:
one HIP launch per direction, the weight and bias gradients formed by torch as one GEMM and one
reduction over all T (``weight_grads``), or with ``fused_wgrad`` by ``weight_grads_fused``: one
``hftlob_xty_wide`` call that reads d_gi, d_gh_n, hseq, h0 and done where they lie.

Notation: ``gi`` [T, B, 3H] is the input projection in gate order (r, z, n), ``done`` [T, B]
resets the carry entering step t, ``h_prev(t) = done[t] ? 0 : (t ? hseq[t-1] : h0)``, and
``gates`` [T, B, 4H] holds (r, z, n, gh_n) of every step.
"""
from __future__ import annotations

import torch

from .. import _lib
from .wgrad import aligned, xty_wide

SUPPORTED_HIDDEN = (64, 128, 256)   # the kernels' template instantiations (csrc/gru_scan.hip)
MAX_GROUPS = 8                      # HFTLOB_GRU_MAX_GROUPS: sequence batches in one grouped launch


def gru_scan_supported(hidden: int) -> bool:
    """Whether the fused scan has a kernel for this hidden size (no GPU needed to ask)."""
    return int(hidden) in SUPPORTED_HIDDEN


def gru_scan_grouped_supported(hidden: int, n_groups: int) -> bool:
    """Whether the grouped scan takes this many groups of this hidden size (no GPU needed to ask)."""
    return gru_scan_supported(hidden) and 1 <= int(n_groups) <= MAX_GROUPS


def _h_prev(hseq, h0, done):
    """h_prev(t) for every t, [T, B, H]."""
    prev = torch.cat([h0[None], hseq[:-1]], 0)
    return torch.where(done.bool()[..., None], torch.zeros_like(prev), prev)


def gru_scan_reference(gi, h0, done, w_hh, b_hh):
    """hftlob_gru_scan_fwd: (hseq [T, B, H], gates [T, B, 4H])."""
    done = done.bool()
    h, hs, gs = h0, [], []
    for t in range(gi.shape[0]):
        h = torch.where(done[t][:, None], torch.zeros_like(h), h)
        ir, iz, i_n = gi[t].chunk(3, -1)
        hr, hz, hn = (h @ w_hh.t() + b_hh).chunk(3, -1)
        r = torch.sigmoid(ir + hr)
        z = torch.sigmoid(iz + hz)
        n = torch.tanh(i_n + r * hn)
        h = (1.0 - z) * n + z * h
        hs.append(h)
        gs.append(torch.cat([r, z, n, hn], -1))
    return torch.stack(hs), torch.stack(gs)


def gru_scan_backward_reference(d_hseq, hseq, gates, h0, done, w_hh):
    """hftlob_gru_scan_bwd: (d_gi [T, B, 3H], d_gh_n [T, B, H], d_h0 [B, H])."""
    done = done.bool()
    hp = _h_prev(hseq, h0, done)
    carry = torch.zeros_like(h0)
    d_gi, d_ghn = [None] * len(hseq), [None] * len(hseq)
    for t in range(len(hseq) - 1, -1, -1):
        r, z, n, ghn = gates[t].chunk(4, -1)
        dh = d_hseq[t] + carry
        dn = dh * (1.0 - z) * (1.0 - n * n)
        dz = dh * (hp[t] - n) * z * (1.0 - z)
        dr = dn * ghn * r * (1.0 - r)
        d_gi[t] = torch.cat([dr, dz, dn], -1)
        d_ghn[t] = dn * r
        dh_prev = dh * z + torch.cat([dr, dz, d_ghn[t]], -1) @ w_hh
        carry = torch.where(done[t][:, None], torch.zeros_like(dh_prev), dh_prev)
    return torch.stack(d_gi), torch.stack(d_ghn), carry


def weight_grads(d_gi, d_gh_n, hseq, h0, done):
    """(d_w_hh [3H, H], d_b_hh [3H]) from the backward operator's outputs: the parts of the
    gradient that are one GEMM and one reduction over all T."""
    H = hseq.shape[-1]
    d_gh = torch.cat([d_gi[..., :2 * H], d_gh_n], -1).reshape(-1, 3 * H)
    return d_gh.t() @ _h_prev(hseq, h0, done).reshape(-1, H), d_gh.sum(0)


def fused_wgrad_operands(d_gi, d_gh_n, hseq, h0, done):
    """``weight_grads`` as the operands of ``wgrad.xty_wide`` / ``xty_wide_reference`` (a_blocks, B, head,
    shift, zero_row), all of them views: d_gh is the first 2H columns of d_gi beside d_gh_n, and h_prev is
    hseq one step (B rows) late behind h0, zeroed where done."""
    T, B, H = hseq.shape
    return ([d_gi.reshape(T * B, 3 * H)[:, :2 * H], d_gh_n.reshape(T * B, H)], hseq.reshape(T * B, H), h0, B,
            done.reshape(T * B))


def weight_grads_fused(d_gi, d_gh_n, hseq, h0, done):
    """(d_w_hh [3H, H], d_b_hh [3H]) as one ``hftlob_xty_wide`` call on contiguous float32 device tensors:
    ``weight_grads`` without its two concatenations and its select."""
    blocks, rows, head, shift, zero_row = fused_wgrad_operands(d_gi, d_gh_n, hseq, h0, done)
    return xty_wide([aligned(a) for a in blocks], aligned(rows), aligned(head), shift, zero_row, want_sum_a=True)


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _u8(done):
    """done as the operators' bytes; a bool tensor is reinterpreted, not copied."""
    done = done.detach().contiguous()
    return done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)


def _fwd_group(name: str, group, save_gates: bool):
    """One group (gi, h0, done, w_hh, b_hh) of a forward launch as the operators take it: the converted
    tensors (they must live until the launch is made), the pointers of those and of the two outputs in the
    operators' argument order, and (hseq, gates or None).  ``name`` heads the shape error."""
    gi, h0, done, w_hh, b_hh = group
    T, B, H3 = gi.shape
    H = H3 // 3
    keep = gi, h0, done, w_hh, b_hh = _f32(gi), _f32(h0), _u8(done), _f32(w_hh), _f32(b_hh)
    if h0.shape != (B, H) or done.shape != (T, B) or w_hh.shape != (3 * H, H) or b_hh.shape != (3 * H,):
        raise ValueError(f"{name}: shapes gi {tuple(gi.shape)}, h0 {tuple(h0.shape)}, done {tuple(done.shape)}, "
                         f"w_hh {tuple(w_hh.shape)}, b_hh {tuple(b_hh.shape)} do not agree")
    hseq = torch.empty((T, B, H), dtype=torch.float32, device=gi.device)
    gates = torch.empty((T, B, 4 * H), dtype=torch.float32, device=gi.device) if save_gates else None
    return keep, [_lib.ptr(x) for x in keep + (hseq, gates)], (hseq, gates)   # (a CPU tensor raises here)


def _bwd_group(name: str, group):
    """``_fwd_group`` for a backward launch: one group (d_hseq, hseq, gates, h0, done, w_hh), the outputs
    (d_gi, d_gh_n, d_h0)."""
    d_hseq, hseq, gates, h0, done, w_hh = group
    T, B, H = hseq.shape
    keep = d_hseq, hseq, gates, h0, done, w_hh = _f32(d_hseq), _f32(hseq), _f32(gates), _f32(h0), _u8(done), _f32(w_hh)
    if d_hseq.shape != (T, B, H) or gates.shape != (T, B, 4 * H) or h0.shape != (B, H) or done.shape != (T, B) \
            or w_hh.shape != (3 * H, H):
        raise ValueError(f"{name}: shapes do not agree")
    out = (torch.empty((T, B, 3 * H), dtype=torch.float32, device=hseq.device),
           torch.empty((T, B, H), dtype=torch.float32, device=hseq.device),
           torch.empty((B, H), dtype=torch.float32, device=hseq.device))
    return keep, [_lib.ptr(x) for x in keep + out], out


def scan_forward(gi, h0, done, w_hh, b_hh, save_gates: bool = True):
    """hftlob_gru_scan_fwd on device tensors: (hseq, gates or None)."""
    keep, ptrs, out = _fwd_group("gru_scan", (gi, h0, done, w_hh, b_hh), save_gates)
    T, B, H = out[0].shape
    _lib.check(_lib.lib().hftlob_gru_scan_fwd(T, B, H, *ptrs, _lib.stream_ptr(device=out[0].device)))
    return out


def scan_backward(d_hseq, hseq, gates, h0, done, w_hh):
    """hftlob_gru_scan_bwd on device tensors: (d_gi, d_gh_n, d_h0)."""
    keep, ptrs, out = _bwd_group("gru_scan backward", (d_hseq, hseq, gates, h0, done, w_hh))
    T, B, H = out[1].shape
    _lib.check(_lib.lib().hftlob_gru_scan_bwd(T, B, H, *ptrs, _lib.stream_ptr(device=out[1].device)))
    return out


class GRUScan(torch.autograd.Function):
    """hseq = gru_scan(gi, h0, done, w_hh, b_hh), differentiable in gi, h0, w_hh and b_hh."""

    @staticmethod
    def forward(ctx, gi, h0, done, w_hh, b_hh, fused_wgrad=False):
        need = any(ctx.needs_input_grad)
        hseq, gates = scan_forward(gi, h0, done, w_hh, b_hh, save_gates=need)
        ctx.fused_wgrad = bool(fused_wgrad)
        if need:
            ctx.save_for_backward(hseq, gates, _f32(h0), done, _f32(w_hh))
        return hseq

    @staticmethod
    def backward(ctx, d_hseq):
        hseq, gates, h0, done, w_hh = ctx.saved_tensors
        # the stream is taken inside the call: autograd runs this under the forward's stream guard
        d_gi, d_gh_n, d_h0 = scan_backward(d_hseq, hseq, gates, h0, done, w_hh)
        d_w, d_b = (None, None)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            d_w, d_b = (weight_grads_fused if ctx.fused_wgrad else weight_grads)(d_gi, d_gh_n, hseq, h0, done)
        return d_gi, d_h0, None, d_w, d_b, None


def gru_scan(gi, h0, done, w_hh, b_hh, fused_wgrad: bool = False):
    """The fused scan: hseq [T, B, H] (float32, on the device of ``gi``).  With ``fused_wgrad`` the backward
    forms W_hh's and b_hh's gradients with ``weight_grads_fused`` instead of ``weight_grads``."""
    return GRUScan.apply(gi, h0, done, w_hh, b_hh, fused_wgrad)


def _check_groups(what: str, shapes) -> tuple:
    """(T, H) of a grouped call from its groups' (T, B, H); raises before anything is launched."""
    shapes = list(shapes)
    if not 1 <= len(shapes) <= MAX_GROUPS:
        raise ValueError(f"{what}: needs 1..{MAX_GROUPS} groups, got {len(shapes)}")
    T, _, H = shapes[0]
    for g, (t, _, h) in enumerate(shapes):
        if (t, h) != (T, H):
            raise ValueError(f"{what}: every group must have the same T and H, group 0 has ({T}, {H}), "
                             f"group {g} ({t}, {h})")
    return T, H


def scan_forward_grouped(groups, save_gates=True):
    """hftlob_gru_scan_fwd_grouped on device tensors: ``groups`` is a sequence of (gi, h0, done, w_hh, b_hh),
    ``save_gates`` a bool or one per group; returns a list of (hseq, gates or None), one launch for all."""
    groups = [tuple(g) for g in groups]
    save = list(save_gates) if isinstance(save_gates, (list, tuple)) else [bool(save_gates)] * len(groups)
    if len(save) != len(groups):
        raise ValueError(f"gru_scan grouped: {len(groups)} groups, {len(save)} save_gates")
    for g in groups:
        if len(g) != 5 or g[0].dim() != 3 or g[0].shape[2] % 3:
            raise ValueError("gru_scan grouped: a group is (gi [T, B, 3H], h0, done, w_hh, b_hh)")
    T, H = _check_groups("gru_scan grouped", [(g[0].shape[0], g[0].shape[1], g[0].shape[2] // 3) for g in groups])
    rows, keep, out = [], [], []
    for k, g in enumerate(groups):
        kept, ptrs, res = _fwd_group(f"gru_scan grouped, group {k}", g, save[k])
        rows.append(_lib.GruFwdGroup(res[0].shape[1], *ptrs))
        keep.append(kept)
        out.append(res)
    arr = (_lib.GruFwdGroup * len(rows))(*rows)
    _lib.check(_lib.lib().hftlob_gru_scan_fwd_grouped(T, H, len(rows), arr, _lib.stream_ptr(device=out[0][0].device)))
    return out


def scan_backward_grouped(groups):
    """hftlob_gru_scan_bwd_grouped on device tensors: ``groups`` is a sequence of (d_hseq, hseq, gates, h0,
    done, w_hh); returns a list of (d_gi, d_gh_n, d_h0), one launch for all."""
    groups = [tuple(g) for g in groups]
    for g in groups:
        if len(g) != 6 or g[1].dim() != 3:
            raise ValueError("gru_scan grouped backward: a group is (d_hseq, hseq [T, B, H], gates, h0, done, w_hh)")
    T, H = _check_groups("gru_scan grouped backward", [tuple(g[1].shape) for g in groups])
    rows, keep, out = [], [], []
    for k, g in enumerate(groups):
        kept, ptrs, res = _bwd_group(f"gru_scan grouped backward, group {k}", g)
        rows.append(_lib.GruBwdGroup(res[1].shape[1], *ptrs))
        keep.append(kept)
        out.append(res)
    arr = (_lib.GruBwdGroup * len(rows))(*rows)
    _lib.check(_lib.lib().hftlob_gru_scan_bwd_grouped(T, H, len(rows), arr, _lib.stream_ptr(device=out[0][0].device)))
    return out


class GRUScanGrouped(torch.autograd.Function):
    """(hseq_0, ..) = gru_scan_grouped over n groups; the inputs are flattened as the n gi, the n h0, the n
    done, the n w_hh and the n b_hh.  Every group is differentiable in its gi, h0, w_hh and b_hh."""

    @staticmethod
    def forward(ctx, n, fused_wgrad, *flat):
        gis, h0s, dones, w_hhs, b_hhs = (flat[k * n:(k + 1) * n] for k in range(5))
        ctx.fused_wgrad = bool(fused_wgrad)
        # (needs_input_grad[0] and [1] are n's and fused_wgrad's)
        need = [any(ctx.needs_input_grad[2 + k * n + g] for k in (0, 1, 3, 4)) for g in range(n)]
        out = scan_forward_grouped(list(zip(gis, h0s, dones, w_hhs, b_hhs)), save_gates=need)
        ctx.n, ctx.need = n, need
        saved = []
        for g in range(n):
            if need[g]:
                saved += [out[g][0], out[g][1], _f32(h0s[g]), dones[g], _f32(w_hhs[g])]
        ctx.save_for_backward(*saved)
        return tuple(hseq for hseq, _ in out)

    @staticmethod
    def backward(ctx, *d_hseqs):
        # (a group whose hseq received no gradient arrives as autograd's materialised zeros)
        n, need, saved = ctx.n, ctx.need, ctx.saved_tensors
        live = [g for g in range(n) if need[g]]
        per = {g: saved[5 * i:5 * i + 5] for i, g in enumerate(live)}
        grads = [None] * (5 * n)
        if live:
            # the stream is taken inside the call: autograd runs this under the forward's stream guard
            res = scan_backward_grouped([(d_hseqs[g],) + tuple(per[g]) for g in live])
            for g, (d_gi, d_gh_n, d_h0) in zip(live, res):
                hseq, _, h0, done, _ = per[g]
                grads[g], grads[n + g] = d_gi, d_h0
                if ctx.needs_input_grad[2 + 3 * n + g] or ctx.needs_input_grad[2 + 4 * n + g]:
                    wg = weight_grads_fused if ctx.fused_wgrad else weight_grads
                    grads[3 * n + g], grads[4 * n + g] = wg(d_gi, d_gh_n, hseq, h0, done)
        return (None, None, *grads)


def gru_scan_grouped(gis, h0s, dones, w_hhs, b_hhs, fused_wgrad: bool = False):
    """The fused scans of several independent nets as one launch per direction: a tuple of hseq [T, B_g, H],
    group g's equal bit for bit to ``gru_scan(gis[g], h0s[g], dones[g], w_hhs[g], b_hhs[g], fused_wgrad)``,
    and so are its gradients (the weight and bias gradients are ``weight_grads`` per group, or with
    ``fused_wgrad`` ``weight_grads_fused``)."""
    lists = [list(x) for x in (gis, h0s, dones, w_hhs, b_hhs)]
    n = len(lists[0])
    if any(len(x) != n for x in lists):
        raise ValueError(f"gru_scan_grouped: the five lists must have one entry per group, got "
                         f"{[len(x) for x in lists]}")
    for gi in lists[0]:
        if gi.dim() != 3 or gi.shape[2] % 3:
            raise ValueError("gru_scan_grouped: gi must be [T, B, 3H]")
    _check_groups("gru_scan_grouped", [(gi.shape[0], gi.shape[1], gi.shape[2] // 3) for gi in lists[0]])
    return GRUScanGrouped.apply(n, bool(fused_wgrad), *(t for x in lists for t in x))
