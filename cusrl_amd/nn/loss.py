"""Loss layers of ``cusrl.nn`` (counterpart of cusrl/nn/layer/loss.py): ``NormalNllLoss`` and ``L2RegularizationLoss``.
``GradientPenaltyLoss`` lives beside its user in ``cusrl_amd/hook/auxiliary/amp.py`` and is re-exported by ``cusrl_amd.nn``.

On fp32 device tensors with a ``"mean"`` or ``"sum"`` reduction both layers are one HIP pass that leaves the loss AND its
gradients (``cusrl_normal_nll_fwd_bwd``, ``cusrl_sumsq_fwd_bwd``) behind an autograd Function whose backward hands the saved
gradients out.  Everything else — ``reduction="none"``, a target that needs a gradient, other dtypes (autocast halves),
broadcasting shapes, CPU tensors — evaluates the reference's torch expression: a loss layer is a building block that user
code may also call on the host, so there is no ``host_form`` gate in front of it."""

from __future__ import annotations

import math
from typing import Literal

import torch
from torch import Tensor, nn

from cusrl_amd.nn.module import saved_gradients

__all__ = ["L2RegularizationLoss", "NormalNllLoss"]

LOG_SQRT_2PI = math.log(2 * math.pi) / 2
_MODES = ("log_var", "log_std", "var", "std")


class _NormalNllFunction(torch.autograd.Function):
    """The reduced loss with the target constant.  ``dist`` None: ``mean`` is the chunked ``[..., 2K]`` input and its gradient
    is the ONE ``[..., 2K]`` tensor the kernel wrote both halves of."""

    @staticmethod
    def forward(ctx, mean, dist, target, mode, full, eps, reduction):
        from cusrl_amd import ops

        loss, d_mean, d_dist = ops.normal_nll_fwd_bwd(mean, dist, target, mode, full, eps, reduction)
        if dist is None:
            ctx.save_for_backward(d_mean._base)
        else:
            ctx.save_for_backward(d_mean, d_dist)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        gradients = saved_gradients(ctx.saved_tensors, grad_loss)
        return gradients[0], (gradients[1] if len(gradients) == 2 else None), None, None, None, None, None


class NormalNllLoss(nn.Module):
    r"""Negative log-likelihood of a Normal distribution given by its mean and a variance parameter.

    ``forward`` takes either a tuple ``(mean, dist)`` or one tensor whose last dimension is split evenly into the two, and a
    target of the mean's shape.  Per element

    .. math::
        \text{loss} = \frac{1}{2} \left( \log \sigma^2 + \frac{(\text{target} - \mu)^2}{\sigma^2} \right)
                      \; \left[ + \frac{1}{2} \log(2\pi) \right]

    Args:
        mode ({"log_var", "log_std", "var", "std"}, optional):
            What the variance parameter holds. Defaults to ``"log_var"``.
        full (bool, optional):
            Adds the constant term. Defaults to ``False``.
        eps (float, optional):
            The variance is clamped from below at this value. Defaults to ``1e-6``.
        reduction ({"none", "mean", "sum"}, optional):
            Reduction applied to the element-wise loss. Defaults to ``"mean"``.
    """

    def __init__(self, *, mode: Literal["log_var", "log_std", "var", "std"] = "log_var", full: bool = False, eps: float = 1e-6,
                 reduction: Literal["none", "mean", "sum"] = "mean") -> None:
        if eps <= 0:
            raise ValueError("'eps' must be greater than zero")
        if mode not in _MODES:
            raise ValueError(f"Unsupported mode '{mode}'; expected one of 'log_var', 'log_std', 'var', or 'std'")
        super().__init__()
        self.mode = mode
        self.full = full
        self.eps = eps
        self.sqrt_eps = math.sqrt(eps)
        self.log_eps = math.log(eps)
        self.reduction = reduction

    def _device_form(self, mean: Tensor, dist: Tensor | None, target: Tensor) -> bool:
        if self.reduction not in ("mean", "sum") or self.mode not in _MODES or not isinstance(target, Tensor):
            return False
        tensors = (mean, target) if dist is None else (mean, dist, target)
        if not all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
            return False
        if target.requires_grad or mean.dim() < 1 or mean.numel() == 0:
            return False
        if dist is None:  # the chunked form: an even last dimension, the target as wide as one half
            return mean.shape[-1] % 2 == 0 and target.shape == (*mean.shape[:-1], mean.shape[-1] // 2)
        return mean.shape == dist.shape == target.shape

    def forward(self, input: Tensor | tuple[Tensor, Tensor], target: Tensor) -> Tensor:
        mean, dist = input if isinstance(input, tuple) else (input, None)
        if self._device_form(mean, dist, target):
            return _NormalNllFunction.apply(mean, dist, target, self.mode, bool(self.full), float(self.eps), self.reduction)
        if dist is None:
            mean, dist = input.chunk(2, dim=-1)
        return self._torch_expression(mean, dist, target)

    def _torch_expression(self, mean: Tensor, dist: Tensor, target: Tensor) -> Tensor:
        if self.mode == "log_var":
            log_var = dist.clamp_min(self.log_eps)
            var = log_var.exp()
        elif self.mode == "log_std":
            log_var = dist.clamp_min(self.log_eps / 2) * 2
            var = log_var.exp()
        elif self.mode == "var":
            var = dist.clamp_min(self.eps)
            log_var = var.log()
        elif self.mode == "std":
            std = dist.clamp_min(self.sqrt_eps)
            var, log_var = std.square(), std.log() * 2
        else:
            raise ValueError(f"Unsupported mode '{self.mode}'")
        nll = 0.5 * (log_var + (target - mean).square() / var)
        if self.full:
            nll = nll + LOG_SQRT_2PI
        return _reduce(nll, self.reduction)


def _reduce(loss: Tensor, reduction: str) -> Tensor:
    if reduction == "mean":
        return loss.mean()
    return loss.sum() if reduction == "sum" else loss


class _SumsqFunction(torch.autograd.Function):
    """``loss_scale * sum(input^2)``; its gradient ``grad_scale * input`` comes from the forward launch."""

    @staticmethod
    def forward(ctx, input, loss_scale, grad_scale):
        from cusrl_amd import ops

        loss, gradient = ops.sumsq_fwd_bwd(input, loss_scale, grad_scale)
        ctx.save_for_backward(gradient)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        return saved_gradients(ctx.saved_tensors, grad_loss)[0], None, None


class L2RegularizationLoss(nn.Module):
    r"""Squared L2 norm of the input, :math:`\text{loss} = \| \text{input} \|_2^2`, element-wise before the reduction.

    Args:
        reduction ({"none", "mean", "sum"}, optional):
            Reduction applied to the squared entries. Defaults to ``"mean"``.
    """

    def __init__(self, reduction: Literal["none", "mean", "sum"] = "mean") -> None:
        super().__init__()
        self.reduction = reduction

    def forward(self, input: Tensor) -> Tensor:
        if self.reduction in ("mean", "sum") and input.is_cuda and input.dtype == torch.float32 and input.numel() > 0:
            scale = 1.0 / input.numel() if self.reduction == "mean" else 1.0
            return _SumsqFunction.apply(input, scale, 2.0 * scale)
        return _reduce(input.square(), self.reduction)
