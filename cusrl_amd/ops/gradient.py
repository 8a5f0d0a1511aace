"""Flat gradient assembly, gradient-norm clipping and the Adam step (``csrc/gradient.hip``)."""

from __future__ import annotations

from collections.abc import Sequence

import torch

from cusrl_amd import _native
from cusrl_amd import ops as _package  # (`assemble_gradients` is looked up there at call time: tests stand in for it on the package)
from cusrl_amd.ops._common import _checked, _f32, _modified_in_place, _ptr, _stream, require_device


def clip_grad_norm_(flat_grad: torch.Tensor, max_norm: float | None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` on one flat fp32 gradient buffer, in place: returns the pre-clip L2 norm
    (0-d device tensor); ``max_norm=None`` only measures (gradient_clipping.py:67-83)."""
    flat_grad = _f32(flat_grad, "flat_grad")
    lib = _native.lib()
    n = flat_grad.numel()
    partials = torch.empty(max(int(lib.cusrl_clip_grad_norm_num_partials(n)), 1), dtype=torch.float64, device=flat_grad.device)
    norm = torch.empty(1, dtype=torch.float32, device=flat_grad.device)
    _checked.cusrl_clip_grad_norm(flat_grad.data_ptr(), n, -1.0 if max_norm is None else float(max_norm),
            partials.data_ptr(), norm.data_ptr(), _stream())
    if max_norm is not None:
        _modified_in_place(flat_grad)  # scaled in place: stale squared-norm partials (FlatGradients.take_sumsq) must not survive
    return norm[0]


class DeferredColumns:
    """Column sums that have NOT been taken yet: ``splits`` partial rows of width ``row_stride`` floats, of which the
    window ``[column, column + numel)`` sums to a gradient.  The column-sum kernels (ReLU-backward + bias gradient,
    narrow-head backward) hand these out instead of running their finalize launch when the flat gradient assembly is
    going to reduce them anyway (``assemble_gradients``)."""

    __slots__ = ("partials", "splits", "row_stride", "column", "numel")

    def __init__(self, partials: torch.Tensor, splits: int, row_stride: int, column: int, numel: int):
        self.partials, self.splits, self.row_stride, self.column, self.numel = partials, splits, row_stride, column, numel

    def materialize(self) -> torch.Tensor:
        out = torch.empty(self.numel, dtype=torch.float32, device=self.partials.device)
        _package.assemble_gradients([(self, 0, self.numel, self.splits)], out)
        return out


def sum_slabs(slabs: torch.Tensor) -> torch.Tensor:
    """``slabs.sum(0)`` of a contiguous ``[S, ...]`` fp32 stack in fixed order through ``cusrl_assemble_gradients`` (one piece):
    no ATen reduction — a global ``reduce_kernel`` brings a semaphore memset node into a captured step."""
    out = torch.empty(slabs.shape[1:], dtype=torch.float32, device=slabs.device)
    if out.numel():
        _package.assemble_gradients([(slabs, 0, out.numel(), slabs.shape[0])], out.view(-1))  # (validates device / dtype / layout)
    return out


def assemble_gradients(pieces: Sequence[tuple], flat: torch.Tensor, want_sumsq: bool = False):
    """Fill the flat gradient buffer in one launch.  ``pieces`` = ``(src, offset, numel, splits)`` per parameter:
    ``src [splits, numel]`` slabs are summed into ``flat[offset : offset + numel]``; ``splits = 1`` copies a plain
    gradient, ``src = None`` / ``splits = 0`` writes zeros; a :class:`DeferredColumns` ``src`` is reduced over its
    partial rows (``splits`` is taken from it).  ``want_sumsq``: also return the blocks' partial sums of squares of what
    they wrote (fp64) — the squared gradient norm :func:`adam_step` turns into the clipping coefficient."""
    flat = _f32(flat, "flat")
    table = (_native.GradPiece * max(len(pieces), 1))()
    keep = []
    for slot, (src, offset, numel, splits) in zip(table, pieces):
        slot.row_stride = 0
        if isinstance(src, DeferredColumns):
            if src.numel != numel or offset < 0 or offset + numel > flat.numel():
                raise ValueError("deferred column sums do not match the parameter's slot")
            keep.append(src.partials)
            slot.src, slot.splits, slot.row_stride = src.partials.data_ptr() + 4 * src.column, src.splits, src.row_stride
        elif src is None or splits == 0:
            slot.src, slot.splits = None, 0
        else:
            src = _f32(src, "gradient piece")
            if src.numel() != splits * numel:
                raise ValueError(f"gradient piece has {src.numel()} elements, expected {splits} x {numel}")
            if offset < 0 or offset + numel > flat.numel():
                raise ValueError("gradient piece does not fit the flat buffer")
            keep.append(src)
            slot.src, slot.splits = src.data_ptr(), splits
        slot.offset, slot.numel = offset, numel
    lib = _native.lib()
    sumsq = None
    if want_sumsq:
        blocks = int(lib.cusrl_assemble_gradients_blocks(table, len(pieces)))
        if 0 < blocks <= 1 << 16:
            sumsq = torch.empty(blocks, dtype=torch.float64, device=flat.device)
    _checked.cusrl_assemble_gradients(table, len(pieces), flat.data_ptr(), _ptr(sumsq), _stream())
    return sumsq


def grad_sumsq(flat_grad: torch.Tensor) -> torch.Tensor:
    """Block partials (double) of ``sum(grad ** 2)`` — the pending norm that :func:`adam_step` turns into the clipping
    coefficient while it streams the gradient."""
    flat_grad = _f32(flat_grad, "flat_grad")
    lib = _native.lib()
    n = flat_grad.numel()
    partials = torch.empty(max(int(lib.cusrl_clip_grad_norm_num_partials(n)), 1), dtype=torch.float64, device=flat_grad.device)
    _checked.cusrl_grad_sumsq(flat_grad.data_ptr(), n, partials.data_ptr(), _stream())
    return partials


def _adam_operands(param, grad, exp_avg, exp_avg_sq, step, lr, ticket, windowed: bool = False, norm_grad=None, workspace=None) -> int:
    """The checks every Adam entry makes of its flat buffers; returns their length.  ``windowed``: the launch covers a window
    of the flat buffers, so the four stretches must be contiguous.  ``norm_grad`` / ``workspace``: those of
    :func:`adam_step_normed`, checked in their places among the others."""
    for tensor, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (step, "step"), (lr, "lr")):
        _f32(tensor, name)
    if norm_grad is not None:
        _f32(norm_grad, "norm_grad")
    require_device(ticket, "ticket")
    if workspace is not None:
        require_device(workspace, "workspace")
    if ticket.dtype != torch.int32 or ticket.numel() != 1:
        raise TypeError("'ticket' must be a 1-element int32 device tensor")
    if workspace is not None and (
            workspace.dtype != torch.uint8 or workspace.numel() < int(_native.lib().cusrl_adam_step_normed_workspace_bytes())):
        raise TypeError("'workspace' comes from ops.adam_norm_workspace")
    n = param.numel()
    same_length = grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == n
    if not windowed:
        if not same_length:
            raise ValueError("flat optimizer buffers must have the same length")
    elif not same_length or not all(
            t.is_contiguous() for t in (param, grad, exp_avg, exp_avg_sq, *(() if norm_grad is None else (norm_grad,)))):
        raise ValueError("a window of the flat optimizer buffers: four contiguous stretches of the same length")
    return n


def adam_step(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
              step: torch.Tensor, lr: torch.Tensor, ticket: torch.Tensor, *, betas: tuple[float, float], eps: float,
              weight_decay: float, decoupled: bool, maximize: bool = False, clip_partials: torch.Tensor | None = None,
              max_norm: float | None = None, norm_out: torch.Tensor | None = None, norm_accumulator: torch.Tensor | None = None):
    """One Adam / AdamW step over flat fp32 buffers, in place (``step`` and ``lr`` are 1-element device tensors).
    ``norm_accumulator`` (a 1-element fp32 view): the pre-clip gradient norm is also added to it."""
    if norm_accumulator is not None:
        _f32(norm_accumulator, "norm_accumulator")
    n = _adam_operands(param, grad, exp_avg, exp_avg_sq, step, lr, ticket)
    _checked.cusrl_adam_step(
        param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), step.data_ptr(), lr.data_ptr(), n,
        float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(decoupled), int(maximize),
        _ptr(clip_partials), 0 if clip_partials is None else clip_partials.numel(),
        -1.0 if max_norm is None else float(max_norm),
        _ptr(norm_out), _ptr(norm_accumulator), ticket.data_ptr(), _stream(),
    )


def adam_step_window(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                     step: torch.Tensor, lr: torch.Tensor, ticket: torch.Tensor, *, betas: tuple[float, float], eps: float,
                     weight_decay: float, decoupled: bool, maximize: bool = False,
                     clip_partials: tuple[torch.Tensor | None, torch.Tensor | None] = (None, None), max_norm: float | None = None,
                     norm_out: torch.Tensor | None = None, norm_accumulator: torch.Tensor | None = None,
                     step_mirror: torch.Tensor | None = None):
    """:func:`adam_step` over one window of the flat buffers (``cusrl_adam_step_window``): ``clip_partials`` = the squared-norm
    partial rows of up to two gradient assemblies, summed as one array; ``step_mirror``: a second counter set to the new count."""
    n = _adam_operands(param, grad, exp_avg, exp_avg_sq, step, lr, ticket, windowed=True)
    first, second = clip_partials
    if any(t is not None and (t.dtype != torch.float64 or not t.is_cuda) for t in (first, second)):
        raise TypeError("'clip_partials' are fp64 device tensors")
    _checked.cusrl_adam_step_window(
        param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), step.data_ptr(), lr.data_ptr(), n,
        float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(decoupled), int(maximize),
        _ptr(first), 0 if first is None else first.numel(), _ptr(second), 0 if second is None else second.numel(),
        -1.0 if max_norm is None else float(max_norm),
        _ptr(norm_out), _ptr(norm_accumulator), _ptr(step_mirror), ticket.data_ptr(), _stream(),
    )


def adam_norm_workspace(device) -> torch.Tensor:
    """A workspace of :func:`adam_step_normed` (0xFF bytes; one per launch that may run beside another one)."""
    return torch.full((int(_native.lib().cusrl_adam_step_normed_workspace_bytes()),), 0xFF, dtype=torch.uint8, device=device)


def adam_step_normed(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                     step: torch.Tensor, lr: torch.Tensor, ticket: torch.Tensor, *, norm_grad: torch.Tensor, workspace: torch.Tensor,
                     betas: tuple[float, float], eps: float, weight_decay: float, decoupled: bool, maximize: bool = False,
                     max_norm: float | None = None, norm_out: torch.Tensor | None = None,
                     norm_accumulator: torch.Tensor | None = None, step_mirror: torch.Tensor | None = None):
    """:func:`adam_step_window` whose launch measures ``||norm_grad||`` itself (``cusrl_adam_step_normed``): the clipping
    coefficient of a step whose gradients were averaged over the ranks after their assembly — no squared-norm launch in between."""
    n = _adam_operands(param, grad, exp_avg, exp_avg_sq, step, lr, ticket, windowed=True, norm_grad=norm_grad, workspace=workspace)
    _checked.cusrl_adam_step_normed(
        param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), step.data_ptr(), lr.data_ptr(), n,
        float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(decoupled), int(maximize),
        norm_grad.data_ptr(), norm_grad.numel(), workspace.data_ptr(), -1.0 if max_norm is None else float(max_norm),
        _ptr(norm_out), _ptr(norm_accumulator), _ptr(step_mirror), ticket.data_ptr(), _stream(),
    )
