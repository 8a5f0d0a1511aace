"""Causal sliding-window attention as HIP launches (the band kernels of ``csrc/attention.hip``): query ``i`` of ``Lq`` sees keys
``i ... i + W`` of ``Lk = Lq + W`` (the first ``W`` are a cache), cut by a key-validity row, by segment ids and biased by ALiBi
slopes — the attention core of the recurrent transformer modules (``nn/causal_attn.py``), on the ``[N, L, H, D]`` layout their
projections leave.  Formulas: include/cusrl_hip.h."""

from __future__ import annotations

import math

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream
from cusrl_amd.ops.attention import (MAX_SDPA_HEAD_DIM, _backward_operands, _differentiated_inside_double_differentiable, _forward_outputs,
                                     _rows_arguments, _rows_layout, sdpa)


def _check_shapes(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from) -> None:
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape:
        raise ValueError(f"band_sdpa: q, k, v must be [N, L, H, D]; got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    N, Lq, H, D = q.shape
    if window < 1 or k.shape != (N, Lq + window, H, D):
        raise ValueError(f"band_sdpa: k and v must be [N, Lq + window, H, D] = {(N, Lq + window, H, D)}; got {tuple(k.shape)}")
    if not 0 <= key_grad_from <= window:
        raise ValueError(f"band_sdpa: 'key_grad_from' must lie in 0 ... window; got {key_grad_from}")
    for name, side, shape in (("key_valid", key_valid, (N, Lq + window)), ("q_segment", q_segment, (N, Lq)), ("alibi_slopes", alibi_slopes, (H,))):
        if side is not None and tuple(side.shape) != shape:
            raise ValueError(f"band_sdpa: '{name}' must have shape {shape}; got {tuple(side.shape)}")


def band_sdpa_supported(q, k, v, window, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0) -> bool:
    """Do the ``cusrl_band_sdpa_*`` entries take this call right now?  fp32 device tensors ``[N, L, H, D]`` on one device with a
    last-dimension stride of 1 and an ``h`` stride of ``D``, ``1 <= D <= CUSRL_MAX_SDPA_HEAD_DIM``, no autocast; ``key_valid``
    bool or uint8, ``q_segment`` int32 and ``alibi_slopes`` fp32, each contiguous on that device and not requiring grad; and —
    when a gradient is asked for — a forward that is not being built inside ``double_differentiable()``."""
    if not all(isinstance(t, torch.Tensor) for t in (q, k, v)) or not q.is_cuda or q.dim() != 4:
        return False
    if any(t.dtype != torch.float32 or t.device != q.device or t.dim() != 4 for t in (q, k, v)):
        return False
    if not 1 <= q.shape[-1] <= MAX_SDPA_HEAD_DIM or torch.is_autocast_enabled("cuda"):
        return False
    if min(q.numel(), k.numel()) < 1 or not all(_rows_layout(t) for t in (q, k, v)):
        return False
    for side, dtypes in ((key_valid, (torch.bool, torch.uint8)), (q_segment, (torch.int32,)), (alibi_slopes, (torch.float32,))):
        if side is None:
            continue
        if not isinstance(side, torch.Tensor) or side.dtype not in dtypes or side.device != q.device:
            return False
        if not side.is_contiguous() or side.requires_grad:
            return False
    return not _differentiated_inside_double_differentiable((q, k, v))


def band_mask(q, window: int, key_valid=None, q_segment=None, alibi_slopes=None) -> torch.Tensor:
    """The band as a dense mask for ``ops.sdpa``: a bool keep-mask ``[N, 1, Lq, Lk]``, or with ALiBi one mask ``[N, H, Lq, Lk]``
    of ``q``'s dtype holding the bias, ``-inf`` where a key is not visible."""
    N, Lq = q.shape[:2]
    Lk = Lq + window
    i = torch.arange(Lq, device=q.device)[:, None]
    j = torch.arange(Lk, device=q.device)[None, :]
    keep = ((j >= i) & (j <= i + window)).expand(N, Lq, Lk)
    if key_valid is not None:
        keep = keep & key_valid.bool()[:, None, :]
    if q_segment is not None:
        kv_segment = torch.cat([q_segment.new_zeros(N, window), q_segment], dim=1)
        keep = keep & (q_segment[:, :, None] == kv_segment[:, None, :])
    if alibi_slopes is None:
        return keep[:, None]
    bias = -alibi_slopes.to(q.dtype)[:, None, None] * (i + window - j).to(q.dtype)
    return bias.expand(N, -1, Lq, Lk).masked_fill(~keep[:, None], -math.inf)


def _side_arguments(key_valid, q_segment, alibi_slopes):
    return _ptr(key_valid), _ptr(q_segment), _ptr(alibi_slopes)


def _launch_band_fwd(q, k, v, window, key_valid=None, q_segment=None, alibi_slopes=None):
    """One ``cusrl_band_sdpa_fwd`` launch: ``(out [N, Lq, H, D], lse [N, H, Lq])``."""
    N, Lq, H, D = q.shape
    out, lse = _forward_outputs(q)
    _checked.cusrl_band_sdpa_fwd(*_rows_arguments(q, k, v), *_side_arguments(key_valid, q_segment, alibi_slopes), 1.0 / math.sqrt(D),
                                 out.data_ptr(), lse.data_ptr(), N, H, Lq, window, D, _stream())
    return out, lse


def band_sdpa_backward(q, k, v, out, lse, dout, window, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0):
    """The ``cusrl_band_sdpa_bwd`` call by itself: ``(dq [N, Lq, H, D], dk, dv [N, Lk - key_grad_from, H, D])``, contiguous; row
    ``j - key_grad_from`` of ``dk`` / ``dv`` is key ``j``'s, and the keys in front of ``key_grad_from`` are not visited."""
    N, Lq, H, D = q.shape
    dout, dq, dk, dv, workspace = _backward_operands(q, dout, Lq + window - key_grad_from,
                                                     _native.lib().cusrl_band_sdpa_bwd_workspace(N, H, Lq, window, D))
    _checked.cusrl_band_sdpa_bwd(*_rows_arguments(q, k, v), *_side_arguments(key_valid, q_segment, alibi_slopes), 1.0 / math.sqrt(D),
                                 out.data_ptr(), lse.data_ptr(), *_rows_arguments(dout), key_grad_from, dq.data_ptr(), dk.data_ptr(),
                                 dv.data_ptr(), workspace.data_ptr(), N, H, Lq, window, D, _stream())
    return dq, dk, dv


def _full_rows(grad: torch.Tensor, key_grad_from: int) -> torch.Tensor:
    """``grad [N, Lk - key_grad_from, H, D]`` as the ``[N, Lk, H, D]`` autograd wants: zeros in front."""
    if key_grad_from == 0:
        return grad
    full = grad.new_zeros((grad.shape[0], grad.shape[1] + key_grad_from, *grad.shape[2:]))
    full[:, key_grad_from:] = grad
    return full


class BandSdpa(torch.autograd.Function):
    """``apply(q, k, v, window, key_valid | None, q_segment | None, alibi_slopes | None, key_grad_from) -> out`` on operands
    :func:`band_sdpa_supported` accepted: one ``cusrl_band_sdpa_fwd`` launch forward, one ``cusrl_band_sdpa_bwd`` call backward.
    Saved: ``q``, ``k``, ``v``, ``out``, ``lse [N, H, Lq]`` and the three small side tensors — nothing of size ``Lq x Lk``.  The
    gradients of ``k`` and ``v`` are zero in front of ``key_grad_from``."""

    @staticmethod
    def forward(ctx, q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from):
        out, lse = _launch_band_fwd(q, k, v, window, key_valid, q_segment, alibi_slopes)
        sides = (key_valid, q_segment, alibi_slopes)
        ctx.save_for_backward(q, k, v, out, lse, *(side for side in sides if side is not None))
        ctx.present = tuple(side is not None for side in sides)
        ctx.window, ctx.key_grad_from = window, key_grad_from
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, *given = ctx.saved_tensors
        given = iter(given)
        sides = [next(given) if present else None for present in ctx.present]
        dq, dk, dv = band_sdpa_backward(q, k, v, out, lse, dout, ctx.window, *sides, key_grad_from=ctx.key_grad_from)
        return dq, _full_rows(dk, ctx.key_grad_from), _full_rows(dv, ctx.key_grad_from), None, None, None, None, None


def band_sdpa(q, k, v, window: int, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0) -> torch.Tensor:
    """Causal sliding-window attention of ``q [N, Lq, H, D]`` over ``k``, ``v`` ``[N, Lq + window, H, D]``, returned as
    ``[N, Lq, H, D]``: query ``i`` sees key ``j`` iff ``i <= j <= i + window``, ``key_valid[n, j]`` and the segment of ``i`` is
    that of ``j`` (``q_segment[n, j - window]``, 0 for the cache); ``alibi_slopes[h] * (i + window - j)`` is taken off the
    scaled score.  Keys in front of ``key_grad_from`` get no gradient.  One launch where :func:`band_sdpa_supported` says so
    (the forward launch alone when no gradient is asked for); everywhere else — CPU tensors, float64, other dtypes, autocast,
    ``D`` beyond the kernel's — the dense mask of :func:`band_mask` through ``ops.sdpa``."""
    _check_shapes(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from)
    if not band_sdpa_supported(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from):
        if key_grad_from > 0 and (k.requires_grad or v.requires_grad):
            k = torch.cat([k[:, :key_grad_from].detach(), k[:, key_grad_from:]], dim=1)
            v = torch.cat([v[:, :key_grad_from].detach(), v[:, key_grad_from:]], dim=1)
        return sdpa(q, k, v, attn_mask=band_mask(q, window, key_valid, q_segment, alibi_slopes))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        return BandSdpa.apply(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from)
    return _launch_band_fwd(q, k, v, window, key_valid, q_segment, alibi_slopes)[0]
