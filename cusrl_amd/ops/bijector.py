"""The bounded sigmoid and the bounded softplus behind a policy's standard deviation as one launch per direction
(``csrc/bijector.hip``).  Formulas: include/cusrl_hip.h."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _stream

_SIGMOID = _native._CONSTANTS["BIJECTOR_SIGMOID"]
_SOFTPLUS = _native._CONSTANTS["BIJECTOR_SOFTPLUS"]


def bijector_supported(x) -> bool:
    """Do the ``cusrl_bijector_*`` entries take this operand right now?  An fp32 device tensor with at least one element, no
    autocast, and — when a gradient is asked for — a forward that is not being built inside ``double_differentiable()`` (the
    backward is once-differentiable).  Everything else (CPU tensors, other dtypes, Python floats) keeps torch's own expression."""
    from cusrl_amd.nn import module

    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.numel() < 1:
        return False
    if torch.is_autocast_enabled("cuda"):
        return False
    return not (torch.is_grad_enabled() and module._plain_linear_depth and x.requires_grad)


def _launch_fwd(x: torch.Tensor, kind: int, params: tuple[float, float, float]) -> torch.Tensor:
    x = x.contiguous()  # (no copy unless a view is strided)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _checked.cusrl_bijector_fwd(kind, x.data_ptr(), out.data_ptr(), x.numel(), *params, _stream())
    return out


class BijectorFunction(torch.autograd.Function):
    """``apply(x, kind, p0, p1, p2) -> y`` on an operand :func:`bijector_supported` accepted: one ``cusrl_bijector_fwd`` launch
    forward, one ``cusrl_bijector_bwd`` launch backward.  Only ``x`` is saved; the backward recomputes from it."""

    @staticmethod
    def forward(ctx, x, kind, p0, p1, p2):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.kind, ctx.params = int(kind), (float(p0), float(p1), float(p2))
        return _launch_fwd(x, ctx.kind, ctx.params)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _checked.cusrl_bijector_bwd(ctx.kind, x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), *ctx.params, _stream())
        return dx, None, None, None, None


def _apply(x: torch.Tensor, kind: int, params: tuple[float, float, float]) -> torch.Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        return BijectorFunction.apply(x, kind, *params)
    return _launch_fwd(x, kind, params)


def sigmoid_bijector(x, min_value: float, max_value: float):
    """``min_value + (max_value - min_value) * sigmoid(x)`` — one launch where :func:`bijector_supported` says so (the forward
    launch alone when no gradient is asked for), torch's own expression, exactly as the reference writes it, everywhere else."""
    value_range = max_value - min_value
    if not bijector_supported(x):
        return min_value + value_range * torch.sigmoid(x)
    return _apply(x, _SIGMOID, (min_value, value_range, 0.0))


def softplus_bijector(x, scale: float, min_input: float, max_input: float):
    """``softplus(clamp(x, min_input, max_input) * scale) / scale`` — one launch where :func:`bijector_supported` says so,
    torch's own expression, exactly as the reference writes it, everywhere else."""
    if not bijector_supported(x):
        return torch.nn.functional.softplus(x.clamp(min_input, max_input) * scale) / scale
    return _apply(x, _SOFTPLUS, (scale, min_input, max_input))
