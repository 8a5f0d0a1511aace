"""Depthwise 2-D convolution as one launch per direction (``csrc/conv.hip``): the spatial half of
``cusrl_amd.nn.SeparableConv2d``.  Formulas: include/cusrl_hip.h."""

from __future__ import annotations

import torch
from torch.nn.functional import conv2d

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream
from cusrl_amd.ops.gate import _launchable


def _pair(value) -> tuple[int, int] | None:
    """``(h, w)`` of an int or a pair of ints, None for anything else."""
    if isinstance(value, int) and not isinstance(value, bool):
        return value, value
    if isinstance(value, (tuple, list)) and len(value) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in value):
        return value[0], value[1]
    return None


def _geometry(weight, stride, padding, dilation) -> tuple[int, ...] | None:
    """``(KH, KW, SH, SW, PH, PW, DH, DW)`` for a ``[C, 1, KH, KW]`` weight, None where the padding does not resolve to one
    integer per axis: ``"valid"`` is 0; ``"same"`` is ``D (K - 1) / 2`` where that is an integer and the stride is 1."""
    if weight.dim() != 4 or weight.shape[1] != 1:
        return None
    KH, KW = weight.shape[2], weight.shape[3]
    stride, dilation = _pair(stride), _pair(dilation)
    if stride is None or dilation is None or min(*stride, *dilation) < 1:
        return None
    if padding == "valid":
        padding = (0, 0)
    elif padding == "same":
        spans = (dilation[0] * (KH - 1), dilation[1] * (KW - 1))
        if stride != (1, 1) or spans[0] % 2 or spans[1] % 2:
            return None
        padding = (spans[0] // 2, spans[1] // 2)
    else:
        padding = _pair(padding)
    if padding is None or min(padding) < 0:
        return None
    return KH, KW, *stride, *padding, *dilation


def _output_shape(x, geometry) -> tuple[int, int, int, int]:
    KH, KW, SH, SW, PH, PW, DH, DW = geometry
    N, C, H, W = x.shape
    return N, C, (H + 2 * PH - DH * (KH - 1) - 1) // SH + 1, (W + 2 * PW - DW * (KW - 1) - 1) // SW + 1


def dwconv2d_supported(x, weight, bias=None, stride=1, padding=0, dilation=1, padding_mode: str = "zeros") -> bool:
    """Do the ``cusrl_dwconv2d_*`` entries take this convolution right now?  The rule of the gate kernels — fp32 device tensors on
    one device, no autocast, and, when a gradient is asked for, a forward that is not being built inside
    ``double_differentiable()`` (the backward is once-differentiable) — for ``x`` ``[N, C, H, W]`` with at least one image and a
    depthwise ``weight`` ``[C, 1, KH, KW]`` of at most ``CUSRL_MAX_DWCONV_TAPS`` taps, ``padding_mode == "zeros"``, and a padding
    that resolves to symmetric integers under which an output exists."""
    tensors = [t for t in (x, weight, bias) if t is not None]
    if padding_mode != "zeros" or len(tensors) < 2 or not _launchable(tensors) or x.dim() != 4:
        return False
    geometry = _geometry(weight, stride, padding, dilation)
    if geometry is None or weight.shape[0] != x.shape[1] or geometry[0] * geometry[1] > _native.MAX_DWCONV_TAPS:
        return False
    if bias is not None and bias.shape != (x.shape[1],):
        return False
    return min(_output_shape(x, geometry)) >= 1


def _launch_fwd(x, weight, bias, geometry) -> torch.Tensor:
    x, weight = x.contiguous(), weight.contiguous()  # (no copy unless a view is strided; a channels_last input is one)
    bias = None if bias is None else bias.contiguous()
    out = torch.empty(_output_shape(x, geometry), dtype=torch.float32, device=x.device)
    _checked.cusrl_dwconv2d_fwd(x.data_ptr(), weight.data_ptr(), _ptr(bias), out.data_ptr(), *x.shape, *geometry, _stream())
    return out


def dwconv2d_backward_input(dout: torch.Tensor, weight: torch.Tensor, input_shape, geometry) -> torch.Tensor:
    """The ``cusrl_dwconv2d_bwd_input`` launch by itself: the gradient of ``x`` ``[N, C, H, W]``; ``geometry`` is
    ``(KH, KW, SH, SW, PH, PW, DH, DW)``.  Positions no window reads are exactly zero."""
    dout, weight = dout.contiguous(), weight.contiguous()
    dx = torch.empty(tuple(input_shape), dtype=torch.float32, device=dout.device)
    _checked.cusrl_dwconv2d_bwd_input(dout.data_ptr(), weight.data_ptr(), dx.data_ptr(), *dx.shape, *geometry, _stream())
    return dx


def dwconv2d_backward_params(x: torch.Tensor, dout: torch.Tensor, geometry, with_bias: bool = True):
    """The ``cusrl_dwconv2d_bwd_params`` call by itself: ``(dw [C, 1, KH, KW], dbias [C] | None)``.  Fixed-order float64 sums:
    the same bits every time."""
    x, dout = x.contiguous(), dout.contiguous()
    N, C, Ho, Wo = dout.shape
    dw = torch.empty(C, 1, geometry[0], geometry[1], dtype=torch.float32, device=x.device)
    dbias = torch.empty(C, dtype=torch.float32, device=x.device) if with_bias else None
    needed = int(_native.lib().cusrl_dwconv2d_num_partials(N, C, Ho, Wo))
    partials = torch.empty(needed, dtype=torch.float64, device=x.device) if needed > 0 else None
    _checked.cusrl_dwconv2d_bwd_params(x.data_ptr(), dout.data_ptr(), dw.data_ptr(), _ptr(dbias), _ptr(partials), *x.shape, *geometry,
                                       _stream())
    return dw, dbias


class DepthwiseConv2d(torch.autograd.Function):
    """``apply(x, weight, bias | None, geometry) -> out`` on operands :func:`dwconv2d_supported` accepted: one
    ``cusrl_dwconv2d_fwd`` launch forward.  Only ``x`` and ``weight`` are saved.  The backward launches
    ``cusrl_dwconv2d_bwd_input`` only where ``x`` wants a gradient (the first layer of an encoder reads observations and does
    not) and ``cusrl_dwconv2d_bwd_params`` only where the weight or the bias does."""

    @staticmethod
    def forward(ctx, x, weight, bias, geometry):
        ctx.geometry, ctx.with_bias = geometry, bias is not None
        ctx.save_for_backward(x, weight)
        return _launch_fwd(x, weight, bias, geometry)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        dx = dw = dbias = None
        if ctx.needs_input_grad[0]:
            dx = dwconv2d_backward_input(dout, weight, x.shape, ctx.geometry)
        if ctx.needs_input_grad[1] or (ctx.with_bias and ctx.needs_input_grad[2]):
            dw, dbias = dwconv2d_backward_params(x, dout, ctx.geometry, with_bias=ctx.with_bias and ctx.needs_input_grad[2])
        return dx, (dw if ctx.needs_input_grad[1] else None), dbias, None


def depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride=1, padding=0, dilation=1) -> torch.Tensor:
    """``conv2d(x, weight, bias, stride, padding, dilation, groups=C)`` with zero padding for a depthwise ``weight``
    ``[C, 1, KH, KW]``: one launch where :func:`dwconv2d_supported` says so (the forward launch alone when no gradient is asked
    for), torch's own convolution everywhere else.  (A ``padding_mode`` other than zeros is the caller's: ``nn.Conv2d`` pads by
    itself before it convolves, ``cusrl_amd.nn.SeparableConv2d`` leaves that to it.)"""
    if not dwconv2d_supported(x, weight, bias, stride, padding, dilation):
        return conv2d(x, weight, bias, stride, padding, dilation, groups=weight.shape[0])
    geometry = _geometry(weight, stride, padding, dilation)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias)):
        return DepthwiseConv2d.apply(x, weight, bias, geometry)
    return _launch_fwd(x, weight, bias, geometry)
