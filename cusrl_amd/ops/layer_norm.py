"""Residual add + LayerNorm as one pass over the row, forward and backward (``csrc/layer_norm.hip``)."""

from __future__ import annotations

import torch
from torch.nn.functional import layer_norm

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream


def add_layer_norm_supported(x: torch.Tensor, residual: torch.Tensor | None, gamma: torch.Tensor | None,
                             beta: torch.Tensor | None) -> bool:
    """Do the ``cusrl_add_layer_norm_*`` entries take these operands right now?  Contiguous fp32 device tensors, rows of 1 to
    ``CUSRL_MAX_LAYER_NORM_WIDTH`` values with an affine LayerNorm over the last dimension, at least one row, no autocast, and —
    when a gradient is asked for — a forward that is not being built inside ``double_differentiable()`` (the backward is
    once-differentiable).  Everything else keeps torch's ``x + residual`` and ``F.layer_norm``."""
    from cusrl_amd.nn import module

    if gamma is None or beta is None or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() < 1:
        return False
    H = x.shape[-1]
    if not 1 <= H <= _native.MAX_LAYER_NORM_WIDTH or x.numel() < H or gamma.shape != (H,) or beta.shape != (H,):
        return False
    if residual is not None and residual.shape != x.shape:
        return False
    operands = [t for t in (x, residual, gamma, beta) if t is not None]
    if any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() for t in operands):
        return False
    if torch.is_autocast_enabled("cuda"):
        return False
    return not (module._plain_linear_depth and torch.is_grad_enabled() and any(t.requires_grad for t in operands))


def add_layer_norm_fwd(x: torch.Tensor, residual: torch.Tensor | None, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                       save_stats: bool = False):
    """One ``cusrl_add_layer_norm_fwd`` launch: ``(s, y, mean, rstd)`` with ``s = x + residual`` (``x`` itself without a
    residual), ``y = LayerNorm(s)`` and, with ``save_stats``, the fp32 row statistics ``[rows]`` the backward reads."""
    H = x.shape[-1]
    rows = x.numel() // H
    s = x if residual is None else torch.empty_like(x)
    y = torch.empty_like(x)
    mean = rstd = None
    if save_stats:
        stats = torch.empty(2, rows, dtype=torch.float32, device=x.device)
        mean, rstd = stats[0], stats[1]
    _checked.cusrl_add_layer_norm_fwd(x.data_ptr(), _ptr(residual), gamma.data_ptr(), beta.data_ptr(), float(eps),
            None if residual is None else s.data_ptr(), y.data_ptr(), _ptr(mean), _ptr(rstd), rows, H, _stream())
    return s, y, mean, rstd


def add_layer_norm_bwd(dy: torch.Tensor, ds: torch.Tensor | None, s: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                       gamma: torch.Tensor):
    """One ``cusrl_add_layer_norm_bwd`` call: ``(d_s, d_gamma, d_beta)``; ``d_s`` = LayerNorm-backward(``dy``) + ``ds`` is the
    gradient of ``x`` and of ``residual`` alike.  Fixed-order float64 column sums: the same bits every time."""
    H = s.shape[-1]
    rows = s.numel() // H
    dy = dy.contiguous()
    ds = None if ds is None else ds.contiguous()
    d_s = torch.empty_like(s)
    d_gamma, d_beta = torch.empty_like(gamma), torch.empty_like(gamma)
    needed = int(_native.lib().cusrl_add_layer_norm_num_partials(rows, H))
    partials = torch.empty(needed, dtype=torch.float64, device=s.device) if needed else None
    _checked.cusrl_add_layer_norm_bwd(dy.data_ptr(), _ptr(ds), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
            d_s.data_ptr(), d_gamma.data_ptr(), d_beta.data_ptr(), _ptr(partials), rows, H, _stream())
    return d_s, d_gamma, d_beta


class AddLayerNorm(torch.autograd.Function):
    """``apply(x, residual | None, gamma, beta, eps) -> (s, y)`` on operands :func:`add_layer_norm_supported` accepted.  The
    backward receives ``(ds, dy)``, makes the one backward call and hands ``d_s`` to ``x`` and ``residual`` both."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps):
        s, y, mean, rstd = add_layer_norm_fwd(x, residual, gamma, beta, eps, save_stats=True)
        ctx.save_for_backward(s, mean, rstd, gamma)
        ctx.has_residual = residual is not None
        ctx.set_materialize_grads(False)
        return s, y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ds, dy):
        s, mean, rstd, gamma = ctx.saved_tensors
        if dy is None:  # nobody used the normalised rows: only the residual stream carries a gradient
            return ds, (ds if ctx.has_residual else None), None, None, None
        d_s, d_gamma, d_beta = add_layer_norm_bwd(dy, ds, s, mean, rstd, gamma)
        return d_s, (d_s if ctx.has_residual else None), d_gamma, d_beta, None


def add_layer_norm(x: torch.Tensor, residual: torch.Tensor | None, gamma: torch.Tensor | None, beta: torch.Tensor | None,
                   eps: float = 1e-5) -> tuple[torch.Tensor, torch.Tensor]:
    """``(s, y)``: ``s = x + residual`` (``x`` without one) and ``y = layer_norm(s)`` over the last dimension — one launch where
    :func:`add_layer_norm_supported` says so, torch's own two operations unchanged everywhere else."""
    if not add_layer_norm_supported(x, residual, gamma, beta):
        s = x if residual is None else x + residual
        return s, layer_norm(s, s.shape[-1:], gamma, beta, eps)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, residual, gamma, beta)):
        return AddLayerNorm.apply(x, residual, gamma, beta, eps)
    s, y, _, _ = add_layer_norm_fwd(x, residual, gamma, beta, eps)
    return s, y
