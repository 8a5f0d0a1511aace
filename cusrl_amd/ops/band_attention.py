"""Causal sliding-window attention as HIP launches (the band kernels of ``csrc/attention.hip``): query ``i`` of ``Lq`` sees keys
``i ... i + W`` of ``Lk = Lq + W`` (the first ``W`` are a cache), cut by a key-validity row, by segment ids and biased by ALiBi
slopes — the attention core of the recurrent transformer modules (``nn/causal_attn.py``), on the ``[N, L, H, D]`` layout their
projections leave; and the one-launch no-grad time step of those modules in input space (``csrc/attention_step.hip``).  Formulas:
include/cusrl_hip.h."""

from __future__ import annotations

import math
import threading
from contextlib import contextmanager

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream, require_device
from cusrl_amd.ops.attention import (MAX_SDPA_HEAD_DIM, _backward_operands, _differentiated_inside_double_differentiable, _forward_outputs,
                                     _matrix_core, _rows_arguments, _rows_layout, _sixteen_byte_rule, sdpa)


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


def band_sdpa_mfma_supported(q, k, v, window, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0) -> bool:
    """Does ``cusrl_band_sdpa_fwd_mfma`` take this call right now?  :func:`band_sdpa_supported`, the shapes the library accepts
    (``cusrl_band_sdpa_fwd_mfma_supported``: ``Lq >= 2``, ``window >= 1``, ``D % 4 == 0``, ``4 <= D <= 128``) and the 16-byte rule
    on ``q``, ``k``, ``v``: every base 16-byte aligned, ``n`` / ``l`` strides multiples of 4."""
    if not band_sdpa_supported(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from):
        return False
    if not _native.lib().cusrl_band_sdpa_fwd_mfma_supported(q.shape[1], window, q.shape[-1]):
        return False
    return _sixteen_byte_rule(q, k, v)


def band_sdpa_bwd_mfma_supported(q, k, v, window, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0) -> bool:
    """Does ``cusrl_band_sdpa_bwd_mfma`` take the backward of this call?  What :func:`band_sdpa_mfma_supported` asks, with the
    library's ``cusrl_band_sdpa_bwd_mfma_supported``; ``out`` and ``dout`` are held to the 16-byte rule when they arrive
    (:func:`band_sdpa_backward`)."""
    if not band_sdpa_supported(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from):
        return False
    if not _native.lib().cusrl_band_sdpa_bwd_mfma_supported(q.shape[1], window, q.shape[-1]):
        return False
    return _sixteen_byte_rule(q, k, v)


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


def _launch_band_fwd(q, k, v, window, key_valid=None, q_segment=None, alibi_slopes=None, matrix_core: bool = False):
    """One ``cusrl_band_sdpa_fwd`` launch (``matrix_core``: one ``cusrl_band_sdpa_fwd_mfma`` launch, on operands
    :func:`band_sdpa_mfma_supported` accepted): ``(out [N, Lq, H, D], lse [N, H, Lq])``."""
    N, Lq, H, D = q.shape
    out, lse = _forward_outputs(q)
    launch = _checked.cusrl_band_sdpa_fwd_mfma if matrix_core else _checked.cusrl_band_sdpa_fwd
    launch(*_rows_arguments(q, k, v), *_side_arguments(key_valid, q_segment, alibi_slopes), 1.0 / math.sqrt(D),
           out.data_ptr(), lse.data_ptr(), N, H, Lq, window, D, _stream())
    return out, lse


def band_sdpa_backward(q, k, v, out, lse, dout, window, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0,
                       matrix_core: bool = False):
    """The ``cusrl_band_sdpa_bwd`` call by itself: ``(dq [N, Lq, H, D], dk, dv [N, Lk - key_grad_from, H, D])``, contiguous; row
    ``j - key_grad_from`` of ``dk`` / ``dv`` is key ``j``'s, and the keys in front of ``key_grad_from`` are not visited.  ``out``
    and ``lse`` are the forward's — either forward's.  ``matrix_core``: the ``cusrl_band_sdpa_bwd_mfma`` call in its place where the
    library takes the shapes and ``q``, ``k``, ``v``, ``out`` and ``dout`` (after the rows-layout copy) pass the 16-byte rule;
    ``cusrl_band_sdpa_bwd`` where not."""
    N, Lq, H, D = q.shape
    dout, dq, dk, dv, workspace = _backward_operands(q, dout, Lq + window - key_grad_from,
                                                     _native.lib().cusrl_band_sdpa_bwd_workspace(N, H, Lq, window, D))
    matrix_core = (bool(matrix_core) and _native.lib().cusrl_band_sdpa_bwd_mfma_supported(Lq, window, D)
                   and _sixteen_byte_rule(q, k, v, out, dout))
    launch = _checked.cusrl_band_sdpa_bwd_mfma if matrix_core else _checked.cusrl_band_sdpa_bwd
    launch(*_rows_arguments(q, k, v), *_side_arguments(key_valid, q_segment, alibi_slopes), 1.0 / math.sqrt(D), out.data_ptr(),
           lse.data_ptr(), *_rows_arguments(dout), key_grad_from, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), workspace.data_ptr(),
           N, H, Lq, window, D, _stream())
    return dq, dk, dv


def _full_rows(grad: torch.Tensor, key_grad_from: int) -> torch.Tensor:
    """``grad [N, Lk - key_grad_from, H, D]`` as the ``[N, Lk, H, D]`` autograd wants: zeros in front."""
    if key_grad_from == 0:
        return grad
    full = grad.new_zeros((grad.shape[0], grad.shape[1] + key_grad_from, *grad.shape[2:]))
    full[:, key_grad_from:] = grad
    return full


class BandSdpa(torch.autograd.Function):
    """``apply(q, k, v, window, key_valid | None, q_segment | None, alibi_slopes | None, key_grad_from[, matrix_core[,
    matrix_core_backward]]) -> out`` on operands :func:`band_sdpa_supported` accepted: one ``cusrl_band_sdpa_fwd`` launch forward
    (``matrix_core``: one ``cusrl_band_sdpa_fwd_mfma`` launch, on operands :func:`band_sdpa_mfma_supported` accepted), one
    ``cusrl_band_sdpa_bwd`` call backward, whichever forward ran (``matrix_core_backward``: one ``cusrl_band_sdpa_bwd_mfma`` call
    where :func:`band_sdpa_backward` finds the operands fit, decided per call when ``dout`` arrives).
    Saved: ``q``, ``k``, ``v``, ``out``, ``lse [N, H, Lq]`` and the three small side tensors — nothing of size ``Lq x Lk``.  The
    gradients of ``k`` and ``v`` are zero in front of ``key_grad_from``."""

    @staticmethod
    def forward(ctx, q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from, matrix_core=False, matrix_core_backward=False):
        out, lse = _launch_band_fwd(q, k, v, window, key_valid, q_segment, alibi_slopes, matrix_core)
        sides = (key_valid, q_segment, alibi_slopes)
        ctx.save_for_backward(q, k, v, out, lse, *(side for side in sides if side is not None))
        ctx.present = tuple(side is not None for side in sides)
        ctx.window, ctx.key_grad_from, ctx.matrix_core_backward = window, key_grad_from, matrix_core_backward
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, *given = ctx.saved_tensors
        given = iter(given)
        sides = [next(given) if present else None for present in ctx.present]
        dq, dk, dv = band_sdpa_backward(q, k, v, out, lse, dout, ctx.window, *sides, key_grad_from=ctx.key_grad_from,
                                        matrix_core=ctx.matrix_core_backward)
        return dq, _full_rows(dk, ctx.key_grad_from), _full_rows(dv, ctx.key_grad_from), None, None, None, None, None, None, None


def band_sdpa(q, k, v, window: int, key_valid=None, q_segment=None, alibi_slopes=None, key_grad_from: int = 0,
              matrix_core: bool | None = None, matrix_core_backward: bool | None = None) -> torch.Tensor:
    """Causal sliding-window attention of ``q [N, Lq, H, D]`` over ``k``, ``v`` ``[N, Lq + window, H, D]``, returned as
    ``[N, Lq, H, D]``: query ``i`` sees key ``j`` iff ``i <= j <= i + window``, ``key_valid[n, j]`` and the segment of ``i`` is
    that of ``j`` (``q_segment[n, j - window]``, 0 for the cache); ``alibi_slopes[h] * (i + window - j)`` is taken off the
    scaled score.  Keys in front of ``key_grad_from`` get no gradient.  One launch where :func:`band_sdpa_supported` says so
    (the forward launch alone when no gradient is asked for); everywhere else — CPU tensors, float64, other dtypes, autocast,
    ``D`` beyond the kernel's — the dense mask of :func:`band_mask` through ``ops.sdpa``.

    ``matrix_core``: True takes the fp32-MFMA forward ``cusrl_band_sdpa_fwd_mfma`` where :func:`band_sdpa_mfma_supported` says so
    and goes on with ``cusrl_band_sdpa_fwd`` where it does not; None (the default) reads the ``enabled`` field of
    ``ops.matrix_core_attention()``, which is off outside the context; False never takes it.  Its results agree with the other
    forward's to rounding, not to the bit (include/cusrl_hip.h).

    ``matrix_core_backward``: the same three values for the backward, independent of ``matrix_core`` (either backward takes
    ``out`` / ``lse`` of either forward): True asks for ``cusrl_band_sdpa_bwd_mfma`` where it is supported and goes on with
    ``cusrl_band_sdpa_bwd`` where not; None reads the context's ``backward`` field; False never takes it."""
    _check_shapes(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from)
    if not band_sdpa_supported(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from):
        if key_grad_from > 0 and (k.requires_grad or v.requires_grad):
            k = torch.cat([k[:, :key_grad_from].detach(), k[:, key_grad_from:]], dim=1)
            v = torch.cat([v[:, :key_grad_from].detach(), v[:, key_grad_from:]], dim=1)
        return sdpa(q, k, v, attn_mask=band_mask(q, window, key_valid, q_segment, alibi_slopes))
    if matrix_core is None:
        matrix_core = getattr(_matrix_core, "enabled", False)
    matrix_core = bool(matrix_core) and band_sdpa_mfma_supported(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from)
    if matrix_core_backward is None:
        matrix_core_backward = getattr(_matrix_core, "backward", False)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        return BandSdpa.apply(q, k, v, window, key_valid, q_segment, alibi_slopes, key_grad_from, matrix_core, bool(matrix_core_backward))
    return _launch_band_fwd(q, k, v, window, key_valid, q_segment, alibi_slopes, matrix_core)[0]


# ------------------------------------------------------------------------------------------- the one-launch acting step
# ``fused_attention_step()``: per thread, whether ``nn.CausalMultiheadSelfAttention`` takes ``cusrl_attn_step_forward`` for a
# no-grad single time step
_fused_step = threading.local()


@contextmanager
def fused_attention_step(enabled: bool = True):
    """Inside the context a no-grad single time step of ``nn.CausalMultiheadSelfAttention`` without RoPE (and of the encoder layer
    built on it) runs as one ``addmm``, one ``cusrl_attn_step_forward`` launch and one ``addmm`` where
    :func:`attention_step_supported` says so, and as it does outside the context where not.  Thread-local, nestable, restored on
    exit."""
    previous = fused_attention_step_enabled()
    _fused_step.enabled = bool(enabled)
    try:
        yield
    finally:
        _fused_step.enabled = previous


def fused_attention_step_enabled() -> bool:
    return getattr(_fused_step, "enabled", False)


def _step_operands(qf, x, cache, cache_mask, alibi_slopes, window, out):
    """``(input pointers, output pointers, (N, H, W, C))`` of a step call, or None when the tensors are not what
    ``cusrl_attn_step_forward`` describes: contiguous fp32 ``qf [N, H, C]``, ``x [N, C]``, ``cache [N, W, C]`` with a bool / uint8
    ``cache_mask [N, W]`` (both None: an empty cache of ``window`` steps), ``alibi_slopes [H]`` or None, all on one device;
    ``out`` = ``(ctx, cache_out, mask_out)`` of the inputs' shapes (``cache_out`` / ``mask_out`` may be None), or None: fresh
    allocations (for the ``_supported`` question a placeholder address, and no roll)."""
    floats = [qf, x, *(t for t in (cache, alibi_slopes) if t is not None), *(t for t in (out or ())[:2] if t is not None)]
    flags = [t for t in (cache_mask, out[2] if out else None) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.device == x.device and t.is_contiguous() for t in (*floats, *flags)):
        return None
    if any(t.dtype != torch.float32 for t in floats) or any(t.dtype not in (torch.bool, torch.uint8) for t in flags):
        return None
    if qf.dim() != 3 or (cache is None) != (cache_mask is None) or (cache is None and window is None):
        return None
    N, H, C = qf.shape
    W = int(window) if cache is None else cache.shape[1]
    if x.shape != (N, C) or (cache is not None and (cache.shape != (N, W, C) or cache_mask.shape != (N, W) or window not in (None, W))):
        return None
    if alibi_slopes is not None and alibi_slopes.shape != (H,):
        return None
    if out is None:
        outputs = (256, None, None)
    else:
        if len(out) != 3 or any(o is not None and o.shape != s for o, s in zip(out, ((N, H, C), (N, W, C), (N, W)))) or out[0] is None:
            return None
        outputs = tuple(_ptr(o) for o in out)
    return (qf.data_ptr(), x.data_ptr(), _ptr(cache), _ptr(cache_mask)), outputs, (N, H, W, C)


def attention_step_supported(qf, x, cache, cache_mask, alibi_slopes=None, window: int | None = None, out=None) -> bool:
    """Does ``cusrl_attn_step_forward`` take these tensors?  The layout of :func:`attention_step_forward`, then asked of the library
    (``cusrl_attn_step_forward_supported``: ``1 <= H <= 16``, ``W >= 1``, ``C % 4 == 0``, ``4 <= C <= 128``, 16-byte aligned
    pointers, no output overlapping an input or another output).  Looks at addresses and sizes only: usable without a GPU."""
    prepared = _step_operands(qf, x, cache, cache_mask, alibi_slopes, window, out)
    if prepared is None:
        return False
    inputs, outputs, sizes = prepared
    return bool(_native.lib().cusrl_attn_step_forward_supported(*inputs, *outputs, *sizes))


def attention_step_forward(qf, x, cache, cache_mask, alibi_slopes=None, scale: float = 1.0, window: int | None = None, out=None):
    """One no-grad time step of causal sliding-window attention in input space as ONE launch (``cusrl_attn_step_forward``;
    formulas: include/cusrl_hip.h): ``(ctx [N, H, C], cache_out [N, W, C], mask_out [N, W])`` for the folded queries
    ``qf [N, H, C]``, the new input ``x [N, C]`` and the window ``cache [N, W, C]`` / ``cache_mask [N, W]`` (both None: an empty
    cache of ``window`` steps).  Head ``h`` attends over the ``W + 1`` raw inputs with score ``(qf[n, h] . X_j) * scale -
    alibi_slopes[h] * (W - j)``; the outputs are the probability-weighted inputs and the window rolled by one step (``mask_out`` in
    ``cache_mask``'s dtype, bool for an empty cache).  ``out``: the three outputs to write (the last two may be None: not
    written), None: fresh tensors.  No autograd.  What the kernel does not take raises."""
    require_device(x, "x")
    if out is None and _step_operands(qf, x, cache, cache_mask, alibi_slopes, window, None) is not None:
        (N, H, C), W = qf.shape, window if cache is None else cache.shape[1]
        out = (torch.empty_like(qf), x.new_empty((N, W, C)),
               torch.empty((N, W), dtype=torch.bool if cache_mask is None else cache_mask.dtype, device=x.device))
    prepared = None if out is None else _step_operands(qf, x, cache, cache_mask, alibi_slopes, window, out)
    if prepared is None:
        raise ValueError("cusrl_attn_step_forward: contiguous fp32 device tensors qf [N, H, C], x [N, C], cache [N, W, C] with a bool / "
                         "uint8 cache_mask [N, W] (or neither, with 'window'), alibi_slopes [H] or None, and outputs of the same shapes")
    inputs, outputs, sizes = prepared
    _checked.cusrl_attn_step_forward(*inputs, _ptr(alibi_slopes), float(scale), *outputs, *sizes, _stream())
    return tuple(out)
