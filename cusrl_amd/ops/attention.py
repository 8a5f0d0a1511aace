"""Scaled dot-product attention and the rotary embedding as HIP launches (``csrc/attention.hip``): one forward launch, one
backward call, on the ``[N, L, H, D]`` layout the attention modules produce — the slices of a packed projection and the
``batch_first=False`` transposition are read where they are.  Formulas: include/cusrl_hip.h."""

from __future__ import annotations

import math
import threading
from contextlib import contextmanager

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
    return not torch.is_autocast_enabled("cuda") and _operands_supported(torch.float32, q, k, v, attn_mask, dropout_p, is_causal)


def _operands_supported(dtype, q, k, v, attn_mask, dropout_p, is_causal) -> bool:
    """What :func:`sdpa_supported` asks of the operands of element type ``dtype``, autocast aside."""
    if not all(isinstance(t, torch.Tensor) for t in (q, k, v)) or not q.is_cuda or q.dim() < 3:
        return False
    if any(t.dtype != dtype or t.device != q.device or t.dim() != q.dim() for t in (q, k, v)):
        return False
    if dropout_p != 0.0 or (attn_mask is not None and is_causal):
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


# ``matrix_core_attention()``: per thread, whether ``sdpa`` calls that leave ``matrix_core=None`` ask for the MFMA forward
# (``enabled``) and those that leave ``matrix_core_backward=None`` for the MFMA backward (``backward``)
_matrix_core = threading.local()


@contextmanager
def matrix_core_attention(enabled: bool = True, backward: bool = False):
    """Inside the context, :func:`sdpa` calls that leave ``matrix_core=None`` behave as ``matrix_core=enabled`` and those that leave
    ``matrix_core_backward=None`` as ``matrix_core_backward=backward`` — how the attention modules reach ``cusrl_sdpa_fwd_mfma`` and
    ``cusrl_sdpa_bwd_mfma`` with no constructor changing: ``with ops.matrix_core_attention(backward=True): layer(x)``.
    Thread-local, nestable, both fields restored on exit."""
    previous = getattr(_matrix_core, "enabled", False), getattr(_matrix_core, "backward", False)
    _matrix_core.enabled, _matrix_core.backward = bool(enabled), bool(backward)
    try:
        yield
    finally:
        _matrix_core.enabled, _matrix_core.backward = previous


def _sixteen_byte_rule(*tensors) -> bool:
    """Every ``[N, L, H, D]`` view's base 16-byte aligned, its ``n`` / ``l`` strides multiples of 4 (fp32) or 8 (bf16) elements."""
    return all(t.data_ptr() % 16 == 0 and t.stride(0) * t.element_size() % 16 == 0 and t.stride(1) * t.element_size() % 16 == 0
               for t in tensors)


def _mfma_supported(entry: str, q, k, v, attn_mask, dropout_p, is_causal) -> bool:
    if not sdpa_supported(q, k, v, attn_mask, dropout_p, is_causal):
        return False
    if not getattr(_native.lib(), entry)(q.shape[-3], k.shape[-3], q.shape[-1]):
        return False
    return _sixteen_byte_rule(*(_one_batch_dimension(t) for t in (q, k, v)))


def sdpa_mfma_supported(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False) -> bool:
    """Does ``cusrl_sdpa_fwd_mfma`` take this call right now?  :func:`sdpa_supported`, the shapes the library accepts
    (``cusrl_sdpa_fwd_mfma_supported``: ``D % 4 == 0``, ``4 <= D <= 128``) and the 16-byte rule on the ``[N, L, H, D]`` views:
    every base 16-byte aligned, ``n`` / ``l`` strides multiples of 4."""
    return _mfma_supported("cusrl_sdpa_fwd_mfma_supported", q, k, v, attn_mask, dropout_p, is_causal)


def sdpa_bwd_mfma_supported(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False) -> bool:
    """Does ``cusrl_sdpa_bwd_mfma`` take the backward of this call?  What :func:`sdpa_mfma_supported` asks, with the library's
    ``cusrl_sdpa_bwd_mfma_supported``; ``dout`` is held to the 16-byte rule when it arrives (:func:`sdpa_backward`)."""
    return _mfma_supported("cusrl_sdpa_bwd_mfma_supported", q, k, v, attn_mask, dropout_p, is_causal)


def sdpa_bf16_supported(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False) -> bool:
    """Does ``cusrl_sdpa_fwd_bf16`` take this call right now?  What :func:`sdpa_supported` asks, of ``torch.bfloat16`` tensors (the
    mask stays bool or fp32), with autocast either off or on with bf16 as its GPU type; the shapes the library accepts
    (``cusrl_sdpa_fwd_bf16_supported``: ``D % 8 == 0``, ``8 <= D <= 128``) and the 16-byte rule on the ``[N, L, H, D]`` views: every
    base 16-byte aligned, ``n`` / ``l`` strides multiples of 8."""
    if not _operands_supported(torch.bfloat16, q, k, v, attn_mask, dropout_p, is_causal):
        return False
    if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") != torch.bfloat16:
        return False
    if not _native.lib().cusrl_sdpa_fwd_bf16_supported(q.shape[-3], k.shape[-3], q.shape[-1]):
        return False
    return _sixteen_byte_rule(*(_one_batch_dimension(t) for t in (q, k, v)))


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


def _launch_sdpa_fwd(q, k, v, mask=None, is_causal: bool = False, matrix_core: bool = False):
    """One ``cusrl_sdpa_fwd`` launch (``matrix_core``: one ``cusrl_sdpa_fwd_mfma`` launch, on operands
    :func:`sdpa_mfma_supported` accepted) on ``[N, L, H, D]`` operands: ``(out [N, Lq, H, D], lse [N, H, Lq])``."""
    N, Lq, H, D = q.shape
    Lk = k.shape[1]
    out, lse = _forward_outputs(q)
    launch = _checked.cusrl_sdpa_fwd_mfma if matrix_core else _checked.cusrl_sdpa_fwd
    launch(*_rows_arguments(q, k, v), *_mask_arguments(mask, N, H, Lq, Lk), int(is_causal), 1.0 / math.sqrt(D),
                            out.data_ptr(), lse.data_ptr(), N, H, Lq, Lk, D, _stream())
    return out, lse


def sdpa_backward(q, k, v, out, lse, dout, mask=None, is_causal: bool = False, matrix_core: bool = False):
    """The ``cusrl_sdpa_bwd`` call by itself: ``(dq, dk, dv)``, contiguous ``[N, L, H, D]``.  ``q``, ``k``, ``v`` and ``dout`` may
    be strided as :func:`sdpa_supported` allows; ``out`` and ``lse`` are the forward's — either forward's.  ``matrix_core``: the
    ``cusrl_sdpa_bwd_mfma`` call in its place where the library takes the shapes and ``q``, ``k``, ``v``, ``out`` and ``dout`` (after
    the rows-layout copy) pass the 16-byte rule; ``cusrl_sdpa_bwd`` where not."""
    N, Lq, H, D = q.shape
    Lk = k.shape[1]
    dout, dq, dk, dv, workspace = _backward_operands(q, dout, Lk, _native.lib().cusrl_sdpa_bwd_workspace(N, H, Lq, Lk, D))
    matrix_core = (bool(matrix_core) and _native.lib().cusrl_sdpa_bwd_mfma_supported(Lq, Lk, D)
                   and _sixteen_byte_rule(q, k, v, out, dout))
    launch = _checked.cusrl_sdpa_bwd_mfma if matrix_core else _checked.cusrl_sdpa_bwd
    launch(*_rows_arguments(q, k, v), out.data_ptr(), lse.data_ptr(), *_rows_arguments(dout), *_mask_arguments(mask, N, H, Lq, Lk),
           int(is_causal), 1.0 / math.sqrt(D), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), workspace.data_ptr(), N, H, Lq, Lk, D,
           _stream())
    return dq, dk, dv


class Sdpa(torch.autograd.Function):
    """``apply(q, k, v, mask | None, is_causal[, matrix_core[, matrix_core_backward]]) -> out`` on ``[N, L, H, D]`` operands
    :func:`sdpa_supported` accepted: one ``cusrl_sdpa_fwd`` launch forward (``matrix_core``: one ``cusrl_sdpa_fwd_mfma`` launch, on
    operands :func:`sdpa_mfma_supported` accepted), one ``cusrl_sdpa_bwd`` call backward (``matrix_core_backward``: one
    ``cusrl_sdpa_bwd_mfma`` call where :func:`sdpa_backward` finds the operands fit, decided per call when ``dout`` arrives).  Saved:
    ``q``, ``k``, ``v``, ``out``, the row statistics ``lse [N, H, Lq]`` and the mask as it was given — nothing of size ``Lq x Lk``;
    the backward recomputes the probabilities."""

    @staticmethod
    def forward(ctx, q, k, v, mask, is_causal, matrix_core=False, matrix_core_backward=False):
        out, lse = _launch_sdpa_fwd(q, k, v, mask, is_causal, matrix_core)
        ctx.save_for_backward(q, k, v, out, lse, *(() if mask is None else (mask,)))
        ctx.is_causal, ctx.matrix_core_backward = is_causal, matrix_core_backward
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, *mask = ctx.saved_tensors
        dq, dk, dv = sdpa_backward(q, k, v, out, lse, dout, mask[0] if mask else None, ctx.is_causal, ctx.matrix_core_backward)
        return dq, dk, dv, None, None, None, None


def _launch_sdpa_fwd_bf16(q, k, v, mask=None, is_causal: bool = False):
    """One ``cusrl_sdpa_fwd_bf16`` launch on bf16 ``[N, L, H, D]`` operands :func:`sdpa_bf16_supported` accepted:
    ``(out [N, Lq, H, D] bf16, lse [N, H, Lq] fp32)``."""
    N, Lq, H, D = q.shape
    Lk = k.shape[1]
    out = torch.empty((N, Lq, H, D), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((N, H, Lq), dtype=torch.float32, device=q.device)
    _checked.cusrl_sdpa_fwd_bf16(*_rows_arguments(q, k, v), *_mask_arguments(mask, N, H, Lq, Lk), int(is_causal), 1.0 / math.sqrt(D),
                                 out.data_ptr(), lse.data_ptr(), N, H, Lq, Lk, D, _stream())
    return out, lse


class SdpaBf16(torch.autograd.Function):
    """``apply(q, k, v, mask | None, is_causal[, matrix_core_backward]) -> out`` on bf16 ``[N, L, H, D]`` operands
    :func:`sdpa_bf16_supported` accepted: one ``cusrl_sdpa_fwd_bf16`` launch forward.  Saved: ``q``, ``k``, ``v``, ``out``, ``lse`` and
    the mask.  There is no bf16 backward kernel: the backward is :func:`sdpa_backward` on fp32 copies of ``q``, ``k``, ``v``, ``out``
    and ``dout`` (``matrix_core_backward`` as in :class:`Sdpa`), its three gradients rounded to bf16 once."""

    @staticmethod
    def forward(ctx, q, k, v, mask, is_causal, matrix_core_backward=False):
        out, lse = _launch_sdpa_fwd_bf16(q, k, v, mask, is_causal)
        ctx.save_for_backward(q, k, v, out, lse, *(() if mask is None else (mask,)))
        ctx.is_causal, ctx.matrix_core_backward = is_causal, matrix_core_backward
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, *mask = ctx.saved_tensors
        with torch.autocast("cuda", enabled=False):
            q, k, v, out, dout = (t.float() for t in (q, k, v, out, dout))
            grads = sdpa_backward(q, k, v, out, lse, dout, mask[0] if mask else None, ctx.is_causal, ctx.matrix_core_backward)
        return (*(g.to(torch.bfloat16) for g in grads), None, None, None)


def sdpa(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False, matrix_core: bool | None = None,
         matrix_core_backward: bool | None = None) -> torch.Tensor:
    """``softmax(q k^T / sqrt(D) + mask) v`` per head on the ``[N, L, H, D]`` layout, returned in the same layout.  One launch
    where :func:`sdpa_supported` says so (the forward launch alone when no gradient is asked for);
    ``F.scaled_dot_product_attention`` on the transposed views everywhere else: CPU tensors, float64, autocast, dropout,
    ``D`` beyond the kernel's, a mask together with ``is_causal``.

    ``matrix_core``: True takes the fp32-MFMA forward ``cusrl_sdpa_fwd_mfma`` where :func:`sdpa_mfma_supported` says so and goes
    on as above where it does not; None (the default) reads :func:`matrix_core_attention`, which is off outside the context;
    False never takes it.  Its results agree with the other forward's to rounding, not to the bit (include/cusrl_hip.h).  On
    ``torch.bfloat16`` tensors - what the attention layers hold under bf16 autocast - True takes ``cusrl_sdpa_fwd_bf16`` where
    :func:`sdpa_bf16_supported` says so (its backward: ``cusrl_sdpa_bwd`` on fp32 copies, the gradients rounded to bf16); without
    it they go to ``F.scaled_dot_product_attention`` as every other non-fp32 call does.

    ``matrix_core_backward``: the same three values for the backward, independent of ``matrix_core`` (either backward takes
    ``out`` / ``lse`` of either forward): True asks for ``cusrl_sdpa_bwd_mfma`` where it is supported and goes on with
    ``cusrl_sdpa_bwd`` where not; None reads the context's ``backward`` field; False never takes it."""
    if matrix_core is None:
        matrix_core = getattr(_matrix_core, "enabled", False)
    if matrix_core_backward is None:
        matrix_core_backward = getattr(_matrix_core, "backward", False)
    if matrix_core and sdpa_bf16_supported(q, k, v, attn_mask, dropout_p, is_causal):
        shape = q.shape
        q, k, v = (_one_batch_dimension(t) for t in (q, k, v))
        if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
            return SdpaBf16.apply(q, k, v, attn_mask, bool(is_causal), bool(matrix_core_backward)).view(shape)
        return _launch_sdpa_fwd_bf16(q, k, v, attn_mask, bool(is_causal))[0].view(shape)
    if not sdpa_supported(q, k, v, attn_mask, dropout_p, is_causal):
        return _sdpa_expression(q, k, v, attn_mask, dropout_p, is_causal)
    matrix_core = bool(matrix_core) and sdpa_mfma_supported(q, k, v, attn_mask, dropout_p, is_causal)
    shape = q.shape
    q, k, v = (_one_batch_dimension(t) for t in (q, k, v))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        out = Sdpa.apply(q, k, v, attn_mask, bool(is_causal), matrix_core, bool(matrix_core_backward))
    else:
        out, _ = _launch_sdpa_fwd(q, k, v, attn_mask, bool(is_causal), matrix_core)
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
