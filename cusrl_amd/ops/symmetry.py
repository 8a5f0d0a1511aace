"""Mirror symmetry: mirrored rows, their gradient, the symmetry loss and symmetric statistics (``csrc/symmetry.hip``)."""

from __future__ import annotations

from collections.abc import Sequence

import torch

from cusrl_amd import _native
from cusrl_amd._native import MirrorField
from cusrl_amd.ops._common import _checked, _f32, _loss_outputs, _modified_in_place, _ptr, _stream, require_device


def _mirror_table(table: torch.Tensor, device: torch.device, c_in: int, c_out: int) -> torch.Tensor:
    """The device reads ``2 C_out + C_in + 1`` entries of a mirror table (include/cusrl_hip.h): checked here, on the host."""
    if table.dtype != torch.int32 or table.dim() != 1 or table.device != device:
        raise TypeError("mirror table: expected the int32 device table of MirrorDef.device_table on the operands' device")
    if table.numel() != 2 * c_out + c_in + 1:
        raise ValueError(f"mirror table: {table.numel()} entries, a map of {c_in} onto {c_out} columns has {2 * c_out + c_in + 1}")
    return table


def _rows_2d(tensor: torch.Tensor, name: str) -> torch.Tensor:
    """``[..., C]`` as a ``[R, C]`` view with unit column stride (a copy only when no such view exists)."""
    require_device(tensor, name)
    if tensor.dtype != torch.float32:
        raise TypeError(f"'{name}' must be float32, got {tensor.dtype}")
    flat = tensor.reshape(-1, tensor.shape[-1]) if tensor.dim() != 2 else tensor
    if flat.shape[1] > 1 and flat.stride(1) != 1 or flat.shape[0] > 1 and flat.stride(0) < flat.shape[1]:
        flat = flat.contiguous()
    return flat


def mirror_rows(fields: Sequence[tuple], rows: int) -> None:
    """One ``cusrl_mirror_rows`` launch.  ``fields``: ``(src [R, C_in], dst [R, ...], dst_offset, mirror)`` with ``mirror`` =
    ``(table, c_in, c_out)`` of ``MirrorDef.device_table`` or None (copy); ``dst``'s rows are written from ``dst_offset``
    on, with ``dst.stride(0)`` between rows (the ``[R, 2, C]`` augmented layout is ``dst.view(R, 2 C)`` at offsets 0 and C)."""
    if not 0 < len(fields) <= _native.MAX_MIRROR_FIELDS:
        raise ValueError(f"mirror_rows: 1 to {_native.MAX_MIRROR_FIELDS} fields per launch, got {len(fields)}")
    table = (MirrorField * len(fields))()
    keep = []
    for i, (src, dst, offset, mirror) in enumerate(fields):
        src = _rows_2d(src, "src")
        require_device(dst, "dst")
        if dst.dtype != torch.float32 or dst.dim() != 2 or (dst.shape[1] > 1 and dst.stride(1) != 1):
            raise TypeError("mirror_rows: dst must be a float32 [R, W] view with unit column stride")
        if src.shape[0] != rows or dst.shape[0] != rows:
            raise ValueError(f"mirror_rows: field {i} has {src.shape[0]} source / {dst.shape[0]} destination rows, expected {rows}")
        if mirror is None:
            width, code = src.shape[1], None
        else:
            code, c_in, width = mirror
            _mirror_table(code, src.device, c_in, width)
            if src.shape[1] != c_in:
                raise ValueError(f"mirror_rows: field {i} is {src.shape[1]} wide, its mirror reads {c_in} columns")
        if offset < 0 or offset + width > dst.shape[1]:
            raise ValueError(f"mirror_rows: field {i} ({width} columns at {offset}) does not fit {dst.shape[1]} columns")
        keep.append(src)
        table[i] = MirrorField(src.data_ptr(), max(src.stride(0), src.shape[1]), dst.data_ptr(), max(dst.stride(0), dst.shape[1]),
                               int(offset), _ptr(code), int(width), int(src.shape[1]))
    _checked.cusrl_mirror_rows(table, len(fields), int(rows), _stream())


def mirror_rows_bwd(grad_out: torch.Tensor, table: torch.Tensor, c_in: int) -> torch.Tensor:
    """Gradient of the mirror: ``grad_out [..., C_out]`` -> ``[..., C_in]`` through the inverse table (fixed-order sums)."""
    lead = grad_out.shape[:-1]
    flat = _rows_2d(grad_out, "grad_out")
    c_out = flat.shape[1]
    _mirror_table(table, flat.device, c_in, c_out)
    grad_in = torch.empty(flat.shape[0], c_in, dtype=torch.float32, device=flat.device)
    _checked.cusrl_mirror_rows_bwd(flat.data_ptr(), max(flat.stride(0), c_out), grad_in.data_ptr(), c_in, table.data_ptr(),
            int(c_in), int(c_out), flat.shape[0], _stream())
    return grad_in.view(*lead, c_in)


def mirror_mse_fwd_bwd(mean: torch.Tensor, mirrored_mean: torch.Tensor, table: torch.Tensor, weight: float,
                       std: torch.Tensor | None = None, mirrored_std: torch.Tensor | None = None):
    """MirrorSymmetryLoss: ``losses [2]`` = weight * (mean((mu - M(mu~))^2), mean((sigma - |M(sigma~)|)^2)) and the gradients
    ``(d_mean, d_mirrored_mean, d_std, d_mirrored_std)`` of their sum, one pass (+ a one-block finalize beyond one block).
    ``std`` / ``mirrored_std``: ``[B, A]`` like the means, or both the ``[A]`` vector the actor repeats; None: no std term."""
    mean, mirrored_mean = _f32(mean, "mean"), _f32(mirrored_mean, "mirrored_mean")
    A = mean.shape[-1]
    if mean.shape != mirrored_mean.shape or mean.numel() == 0:
        raise ValueError("mirror_mse_fwd_bwd: the two means differ in shape or are empty")
    _mirror_table(table, mean.device, A, A)  # (the action mirror maps A columns onto A)
    B = mean.numel() // A
    vector = False
    if std is not None:
        std, mirrored_std = _f32(std, "std"), _f32(mirrored_std, "mirrored_std")
        if std.shape != mirrored_std.shape:
            raise ValueError("mirror_mse_fwd_bwd: std and mirrored_std differ in shape")
        vector = std.dim() == 1
        if (std.shape != (A,)) if vector else (std.shape != mean.shape):
            raise ValueError(f"mirror_mse_fwd_bwd: std must be [A] or shaped like the mean, got {tuple(std.shape)}")
    losses, partials = _loss_outputs(mean.device, _native.lib().cusrl_mirror_mse_num_partials(B * A), terms=2)
    d_mean, d_mirrored = torch.empty_like(mean), torch.empty_like(mean)
    d_std = None if std is None else torch.empty_like(std)
    d_mirrored_std = None if std is None else torch.empty_like(std)
    _checked.cusrl_mirror_mse_fwd_bwd(mean.data_ptr(), mirrored_mean.data_ptr(), _ptr(std), _ptr(mirrored_std), int(vector),
            table.data_ptr(), B, A, float(weight), losses.data_ptr(), d_mean.data_ptr(), d_mirrored.data_ptr(), _ptr(d_std),
            _ptr(d_mirrored_std), partials.data_ptr(), _stream())
    return losses, d_mean, d_mirrored, d_std, d_mirrored_std


def symmetrize_mean_var_(mean: torch.Tensor, var: torch.Tensor, table: torch.Tensor) -> None:
    """observation.py:213-217 in place on fp32 ``mean`` / ``var [C]`` (one launch, the reference's fp32 rounding order)."""
    for t, name in ((mean, "mean"), (var, "var")):
        require_device(t, name)
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise TypeError(f"symmetrize_mean_var_: '{name}' must be a contiguous float32 vector")
    C = mean.numel()
    if var.numel() != C:
        raise ValueError("symmetrize_mean_var_: mean and var differ in size")
    _mirror_table(table, mean.device, C, C)  # (the mirror maps C columns onto C)
    _checked.cusrl_symmetrize_mean_var(mean.data_ptr(), var.data_ptr(), table.data_ptr(), C, _stream())
    _modified_in_place(mean)
    _modified_in_place(var)
