"""Scaled dot-product attention and the rotary embedding as HIP launches (``csrc/attention.hip``): one forward launch, one
backward call, on the ``[N, L, H, D]`` layout the attention modules produce — the slices of a packed projection and the
``batch_first=False`` transposition are read where they are.  Formulas: include/cusrl_hip.h."""

from __future__ import annotations

import math

import torch
from torch.nn.functional import scaled_dot_product_attention

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream

MAX_SDPA_HEAD_DIM = _native._CONSTANTS["MAX_SDPA_HEAD_DIM"]


def _differentiated_inside_double_differentiable(tensors) -> bool:
    from cusrl_amd.nn import module

    return bool(torch.is_grad_enabled() and module._plain_linear_depth and any(t.requires_grad for t in tensors))


def _rows_layout(t: torch.Tensor) -> bool:
    """``[..., L, H, D]`` with element ``(l, h, d)`` at ``l * stride_l + h * D + d``."""
    return t.stride(-1) == 1 and t.stride(-2) == t.shape[-1]


def _one_batch_dimension(t: torch.Tensor) -> torch.Tensor | None:
    """``t`` ``[..., L, H, D]`` as ``[N, L, H, D]`` where that is a view; None where it would be a copy."""
    if t.dim() == 4:
        return t
    if t.dim() == 3:
        return t.unsqueeze(0)
    try:
        return t.view(-1, *t.shape[-3:])
    except RuntimeError:
        return None


def _mask_strides(mask, N, H, Lq, Lk):
    return (0, 0, 0, 0) if mask is None else mask.expand(N, H, Lq, Lk).stride()


def sdpa_supported(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False) -> bool:
    """Do the ``cusrl_sdpa_*`` entries take this call right now?  fp32 device tensors ``[N, L, H, D]`` on one device with a
    last-dimension stride of 1 and an ``h`` stride of ``D``, ``1 <= D <= CUSRL_MAX_SDPA_HEAD_DIM``, no autocast, no dropout, not
    a mask and ``is_causal`` together, a bool or fp32 mask that does not require grad and broadcasts to ``(N, H, Lq, Lk)``, and
    — when a gradient is asked for — a forward that is not being built inside ``double_differentiable()``.  Other leading
    dimensions are accepted where folding them into one is a view and no mask is given."""
    if not all(isinstance(t, torch.Tensor) for t in (q, k, v)) or not q.is_cuda or q.dim() < 3:
        return False
    if any(t.dtype != torch.float32 or t.device != q.device or t.dim() != q.dim() for t in (q, k, v)):
        return False
    if dropout_p != 0.0 or (attn_mask is not None and is_causal) or torch.is_autocast_enabled("cuda"):
        return False
    if q.dim() != 4 and attn_mask is not None:
        return False
    D = q.shape[-1]
    if not 1 <= D <= MAX_SDPA_HEAD_DIM or k.shape[-2:] != q.shape[-2:] or v.shape != k.shape or k.shape[:-3] != q.shape[:-3]:
        return False
    if min(q.numel(), k.numel()) < 1 or not all(_rows_layout(t) for t in (q, k, v)):
        return False
    if any(_one_batch_dimension(t) is None for t in (q, k, v)):
        return False
    if attn_mask is not None:
        if not isinstance(attn_mask, torch.Tensor) or attn_mask.dtype not in (torch.bool, torch.float32):
            return False
        if attn_mask.device != q.device or attn_mask.requires_grad or attn_mask.dim() > 4:
            return False
        full = (q.shape[0], q.shape[2], q.shape[1], k.shape[1])
        try:
            if tuple(torch.broadcast_shapes(attn_mask.shape, full)) != full:
                return False
        except RuntimeError:
            return False
    return not _differentiated_inside_double_differentiable((q, k, v))


def _sdpa_expression(q, k, v, attn_mask, dropout_p, is_causal):
    """The reference's call (cusrl/nn/layer/mha.py:133-140), so every error is torch's own."""
    return scaled_dot_product_attention(q.transpose(-2, -3), k.transpose(-2, -3), v.transpose(-2, -3), attn_mask=attn_mask,
                                        dropout_p=dropout_p, is_causal=is_causal).transpose(-2, -3)


def _mask_arguments(mask, N, H, Lq, Lk):
    keep = mask if mask is not None and mask.dtype == torch.bool else None
    bias = mask if mask is not None and mask.dtype != torch.bool else None
    return (_ptr(keep), _ptr(bias), *_mask_strides(mask, N, H, Lq, Lk))


def _rows_arguments(*tensors):
    """``(data_ptr, stride_n, stride_l)`` of each ``[N, L, H, D]`` tensor, as the entries take them."""
    return tuple(a for t in tensors for a in (t.data_ptr(), t.stride(0), t.stride(1)))


def _forward_outputs(q):
    """``(out [N, Lq, H, D], lse [N, H, Lq])`` for a forward launch to fill."""
    N, Lq, H, D = q.shape
    return (torch.empty((N, Lq, H, D), dtype=torch.float32, device=q.device),
            torch.empty((N, H, Lq), dtype=torch.float32, device=q.device))


def _backward_operands(q, dout, key_rows: int, workspace_floats: int):
    """``dout`` in the rows layout (a copy where it is not), then what a backward call fills: ``dq [N, Lq, H, D]``, ``dk`` and
    ``dv`` ``[N, key_rows, H, D]`` and the fp32 workspace."""
    N, Lq, H, D = q.shape
    if not _rows_layout(dout):
        dout = dout.contiguous()
    dq, dk, dv = (torch.empty((N, rows, H, D), dtype=torch.float32, device=q.device) for rows in (Lq, key_rows, key_rows))
    return dout, dq, dk, dv, torch.empty(int(workspace_floats), dtype=torch.float32, device=q.device)


def _launch_sdpa_fwd(q, k, v, mask=None, is_causal: bool = False):
    """One ``cusrl_sdpa_fwd`` launch on ``[N, L, H, D]`` operands: ``(out [N, Lq, H, D], lse [N, H, Lq])``."""
    N, Lq, H, D = q.shape
    Lk = k.shape[1]
    out, lse = _forward_outputs(q)
    _checked.cusrl_sdpa_fwd(*_rows_arguments(q, k, v), *_mask_arguments(mask, N, H, Lq, Lk), int(is_causal), 1.0 / math.sqrt(D),
                            out.data_ptr(), lse.data_ptr(), N, H, Lq, Lk, D, _stream())
    return out, lse


def sdpa_backward(q, k, v, out, lse, dout, mask=None, is_causal: bool = False):
    """The ``cusrl_sdpa_bwd`` call by itself: ``(dq, dk, dv)``, contiguous ``[N, L, H, D]``.  ``q``, ``k``, ``v`` and ``dout`` may
    be strided as :func:`sdpa_supported` allows; ``out`` and ``lse`` are the forward's."""
    N, Lq, H, D = q.shape
    Lk = k.shape[1]
    dout, dq, dk, dv, workspace = _backward_operands(q, dout, Lk, _native.lib().cusrl_sdpa_bwd_workspace(N, H, Lq, Lk, D))
    _checked.cusrl_sdpa_bwd(*_rows_arguments(q, k, v), out.data_ptr(), lse.data_ptr(), *_rows_arguments(dout),
                            *_mask_arguments(mask, N, H, Lq, Lk), int(is_causal), 1.0 / math.sqrt(D), dq.data_ptr(), dk.data_ptr(),
                            dv.data_ptr(), workspace.data_ptr(), N, H, Lq, Lk, D, _stream())
    return dq, dk, dv


class Sdpa(torch.autograd.Function):
    """``apply(q, k, v, mask | None, is_causal) -> out`` on ``[N, L, H, D]`` operands :func:`sdpa_supported` accepted: one
    ``cusrl_sdpa_fwd`` launch forward, one ``cusrl_sdpa_bwd`` call backward.  Saved: ``q``, ``k``, ``v``, ``out``, the row
    statistics ``lse [N, H, Lq]`` and the mask as it was given — nothing of size ``Lq x Lk``; the backward recomputes the
    probabilities."""

    @staticmethod
    def forward(ctx, q, k, v, mask, is_causal):
        out, lse = _launch_sdpa_fwd(q, k, v, mask, is_causal)
        ctx.save_for_backward(q, k, v, out, lse, *(() if mask is None else (mask,)))
        ctx.is_causal = is_causal
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, *mask = ctx.saved_tensors
        dq, dk, dv = sdpa_backward(q, k, v, out, lse, dout, mask[0] if mask else None, ctx.is_causal)
        return dq, dk, dv, None, None


def sdpa(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False) -> torch.Tensor:
    """``softmax(q k^T / sqrt(D) + mask) v`` per head on the ``[N, L, H, D]`` layout, returned in the same layout.  One launch
    where :func:`sdpa_supported` says so (the forward launch alone when no gradient is asked for);
    ``F.scaled_dot_product_attention`` on the transposed views everywhere else: CPU tensors, float64, autocast, dropout,
    ``D`` beyond the kernel's, a mask together with ``is_causal``."""
    if not sdpa_supported(q, k, v, attn_mask, dropout_p, is_causal):
        return _sdpa_expression(q, k, v, attn_mask, dropout_p, is_causal)
    shape = q.shape
    q, k, v = (_one_batch_dimension(t) for t in (q, k, v))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        out = Sdpa.apply(q, k, v, attn_mask, bool(is_causal))
    else:
        out, _ = _launch_sdpa_fwd(q, k, v, attn_mask, bool(is_causal))
    return out.view(shape)


# ---------------------------------------------------------------------------------------------------------------- RoPE
def rope_supported(x, cos, sin) -> bool:
    """Does ``cusrl_rope_apply`` take these operands right now?  ``x`` fp32 on the device, ``[..., L, H, D]`` with ``D`` even, a
    last-dimension stride of 1 and an ``h`` stride of ``D``, leading dimensions that fold into one as a view; ``cos`` / ``sin``
    contiguous fp32 ``[L, D / 2]`` there, not requiring grad; no autocast, not a differentiated forward inside
    ``double_differentiable()``."""
    if not all(isinstance(t, torch.Tensor) for t in (x, cos, sin)) or not x.is_cuda or x.dim() < 3 or x.numel() < 1:
        return False
    L, _, D = x.shape[-3:]
    if D % 2 or any(t.dtype != torch.float32 or t.device != x.device for t in (x, cos, sin)):
        return False
    if any(t.shape != (L, D // 2) or not t.is_contiguous() or t.requires_grad for t in (cos, sin)):
        return False
    if not _rows_layout(x) or _one_batch_dimension(x) is None or torch.is_autocast_enabled("cuda"):
        return False
    return not _differentiated_inside_double_differentiable((x,))


def _rope_expression(x, cos, sin):
    """cusrl/nn/layer/encoding.py:107-125."""
    cos, sin = cos.repeat(1, 2).unsqueeze(-2), sin.repeat(1, 2).unsqueeze(-2)
    first, second = x.chunk(2, dim=-1)
    return x * cos + torch.cat((-second, first), dim=-1) * sin


def _launch_rope(x, cos, sin, transpose: bool) -> torch.Tensor:
    """One ``cusrl_rope_apply`` launch on ``x [N, L, H, D]``; ``transpose``: the backward's map."""
    N, L, H, D = x.shape
    out = torch.empty((N, L, H, D), dtype=torch.float32, device=x.device)
    _checked.cusrl_rope_apply(x.data_ptr(), x.stride(0), x.stride(1), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), N, L, H, D,
                              int(transpose), _stream())
    return out


class Rope(torch.autograd.Function):
    """``apply(x, cos, sin) -> out`` on operands :func:`rope_supported` accepted: one ``cusrl_rope_apply`` launch each way (the
    backward is the transposed rotation of ``dout``).  Saved: the ``cos`` / ``sin`` rows."""

    @staticmethod
    def forward(ctx, x, cos, sin):
        ctx.save_for_backward(cos, sin)
        return _launch_rope(x, cos, sin, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        cos, sin = ctx.saved_tensors
        return _launch_rope(dout if _rows_layout(dout) else dout.contiguous(), cos, sin, True), None, None


def rope(x, cos, sin) -> torch.Tensor:
    """``x cos + rotate_half(x) sin`` over ``x [..., L, H, D]`` with the ``[L, D / 2]`` rows of the rotary cache: one launch where
    :func:`rope_supported` says so, the reference's torch expression everywhere else."""
    if not rope_supported(x, cos, sin):
        return _rope_expression(x, cos, sin)
    shape = x.shape
    x = _one_batch_dimension(x)
    out = Rope.apply(x, cos, sin) if torch.is_grad_enabled() and x.requires_grad else _launch_rope(x, cos, sin, False)
    return out.view(shape)
