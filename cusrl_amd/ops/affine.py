"""A per-column affine map with fixed statistics as one launch, forward and backward (``csrc/column_affine.hip``):
``(x - mean) / std`` and its inverse ``x * std + mean``, bit-identical to torch's fp32 expressions."""

from __future__ import annotations

import torch

from cusrl_amd.ops._common import _checked, _stream


def column_affine_supported(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> bool:
    """Do the ``cusrl_column_affine_*`` entries take these operands right now?  fp32 device tensors with ``C`` columns in the last
    dimension of ``x`` and ``mean`` / ``std`` of shape ``(C,)``, at least one row, no autocast, and — when a gradient is asked
    for — a forward that is not being built inside ``double_differentiable()`` (the backward is once-differentiable) and
    statistics that ask for none (there is no column reduction).  Everything else keeps torch's own expression."""
    from cusrl_amd.nn import module

    operands = (x, mean, std)
    if not all(isinstance(t, torch.Tensor) for t in operands) or not x.is_cuda or x.dim() < 1 or mean.dim() != 1:
        return False
    C = mean.shape[0]
    if C < 1 or x.shape[-1] != C or std.shape != (C,) or x.numel() < C:
        return False
    if any(t.dtype != torch.float32 or t.device != x.device for t in operands):
        return False
    if torch.is_autocast_enabled("cuda"):
        return False
    if not torch.is_grad_enabled():
        return True
    return not (mean.requires_grad or std.requires_grad or (module._plain_linear_depth and x.requires_grad))


def _launch_fwd(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, inverse: bool) -> torch.Tensor:
    x, mean, std = x.contiguous(), mean.contiguous(), std.contiguous()  # (no copy unless a view is strided)
    C = mean.shape[0]
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _checked.cusrl_column_affine_fwd(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), x.numel() // C, C,
                                     int(inverse), _stream())
    return out


class ColumnAffine(torch.autograd.Function):
    """``apply(x, mean, std, inverse) -> out`` on operands :func:`column_affine_supported` accepted: one
    ``cusrl_column_affine_fwd`` launch forward, one ``cusrl_column_affine_bwd`` launch backward (``dy / std``, or ``dy * std``
    for the inverse).  Only ``std`` is saved; ``mean`` and ``std`` receive no gradient."""

    @staticmethod
    def forward(ctx, x, mean, std, inverse):
        ctx.save_for_backward(std)
        ctx.inverse = bool(inverse)
        return _launch_fwd(x, mean, std, ctx.inverse)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (std,) = ctx.saved_tensors
        dy, std = dy.contiguous(), std.contiguous()
        C = std.shape[0]
        dx = torch.empty(dy.shape, dtype=torch.float32, device=dy.device)
        _checked.cusrl_column_affine_bwd(dy.data_ptr(), std.data_ptr(), dx.data_ptr(), dy.numel() // C, C, int(ctx.inverse),
                                         _stream())
        return dx, None, None, None


def column_affine(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """``(x - mean) / std``, or with ``inverse`` ``x * std + mean``, over the last dimension — one launch where
    :func:`column_affine_supported` says so (the forward launch alone when no gradient is asked for), torch's own expression,
    exactly as the reference writes it, everywhere else."""
    if not column_affine_supported(x, mean, std):
        return x * std + mean if inverse else (x - mean) / std
    if torch.is_grad_enabled() and x.requires_grad:
        return ColumnAffine.apply(x, mean, std, inverse)
    return _launch_fwd(x, mean, std, bool(inverse))
