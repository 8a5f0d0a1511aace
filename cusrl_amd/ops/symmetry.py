"""Mirror symmetry: mirrored rows, their gradient, the symmetry loss, symmetric statistics and the head of a symmetric actor
(``csrc/symmetry.hip``)."""

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


def symmetric_head_supported(rows: int, actions: int) -> bool:
    """The shape limits of the ``cusrl_symmetric_head_*`` entries (include/cusrl_hip.h) for ``rows`` combined rows."""
    return 1 <= actions <= _native.MAX_SYMMETRIC_HEAD_ACTIONS and 0 <= 2 * rows * actions <= 2**31 - 1


def _stacked_head(mean2: torch.Tensor, std2: torch.Tensor, table: torch.Tensor, who: str):
    """``(mean2, std2, std is a vector, B, A)`` of the stacked head outputs: ``mean2 [2B, A]``, ``std2`` like it or ``[A]``."""
    if mean2.dim() != 2 or mean2.shape[0] % 2:
        raise ValueError(f"{who}: the stacked mean must be [2B, A], got {tuple(mean2.shape)}")
    A = mean2.shape[1]
    vector = std2.dim() == 1
    if (std2.shape != (A,)) if vector else (std2.shape != mean2.shape):
        raise ValueError(f"{who}: std must be [A] or shaped like the stacked mean, got {tuple(std2.shape)}")
    _mirror_table(table, mean2.device, A, A)  # (the action mirror maps A columns onto A; checked before anything is launched)
    return _f32(mean2, "mean2"), _f32(std2, "std2"), vector, mean2.shape[0] // 2, A


def symmetric_head_fwd(mean2: torch.Tensor, std2: torch.Tensor, table: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(mean, std) [B, A]`` of a symmetric actor from the stacked head outputs (original rows first, mirrored rows second):
    ``(mean_o + M(mean_m)) / 2`` and ``(std_o + |M(std_m)|) / 2``, one launch, bit-identical to the torch expression."""
    mean2, std2, vector, B, A = _stacked_head(mean2, std2, table, "symmetric_head_fwd")
    mean, std = (torch.empty(B, A, dtype=torch.float32, device=mean2.device) for _ in range(2))
    _checked.cusrl_symmetric_head_fwd(mean2.data_ptr(), std2.data_ptr(), int(vector), table.data_ptr(), B, A, mean.data_ptr(),
            std.data_ptr(), _stream())
    return mean, std


def symmetric_head_sample(mean2: torch.Tensor, std2: torch.Tensor, table: torch.Tensor, eps: torch.Tensor):
    """The acting step behind the stacked pass, one launch: ``(action, logp [B, 1], mean, std)`` with ``action = mean + std * eps``
    and the Normal log-probability of it summed over the action."""
    mean2, std2, vector, B, A = _stacked_head(mean2, std2, table, "symmetric_head_sample")
    eps = _f32(eps, "eps")
    if eps.shape != (B, A):
        raise ValueError(f"symmetric_head_sample: eps must be {(B, A)}, got {tuple(eps.shape)}")
    action, mean, std = (torch.empty(B, A, dtype=torch.float32, device=mean2.device) for _ in range(3))
    logp = torch.empty(B, 1, dtype=torch.float32, device=mean2.device)
    _checked.cusrl_symmetric_head_sample(mean2.data_ptr(), std2.data_ptr(), int(vector), eps.data_ptr(), table.data_ptr(), B, A,
            action.data_ptr(), logp.data_ptr(), mean.data_ptr(), std.data_ptr(), _stream())
    return action, logp, mean, std


def symmetric_head_bwd(g_mean: torch.Tensor | None, g_std: torch.Tensor | None, std2: torch.Tensor, table: torch.Tensor,
                       want_bias: bool = False):
    """Gradient of :func:`symmetric_head_fwd`: ``(d_mean2 [2B, A] | None, d_std2 shaped like std2 | None, d_bias [A] | None)``
    from ``g_mean`` / ``g_std [B, A]`` (None: that gradient is not asked for).  ``want_bias``: also the gradient of a head bias
    inside ``mean2`` (the column sums of ``d_mean2``, the two halves paired row by row: exactly 0 where they cancel).
    Fixed-order sums, no atomics: the same bits every time."""
    given = g_mean if g_mean is not None else g_std
    if given is None:
        raise ValueError("symmetric_head_bwd: neither gradient is given")
    if given.dim() != 2 or any(g is not None and g.shape != given.shape for g in (g_mean, g_std)):
        raise ValueError("symmetric_head_bwd: the incoming gradients must be [B, A]")
    B, A = given.shape
    vector = std2.dim() == 1
    if (std2.shape != (A,)) if vector else (std2.shape != (2 * B, A)):
        raise ValueError(f"symmetric_head_bwd: std must be [A] or [2B, A], got {tuple(std2.shape)}")
    _mirror_table(table, given.device, A, A)
    g_mean = None if g_mean is None else _f32(g_mean, "g_mean")
    g_std = None if g_std is None else _f32(g_std, "g_std")
    std2 = _f32(std2, "std2")
    d_mean2 = None if g_mean is None else torch.empty(2 * B, A, dtype=torch.float32, device=given.device)
    d_std2 = None if g_std is None else torch.empty_like(std2)
    want_bias = want_bias and g_mean is not None
    d_bias = torch.empty(A, dtype=torch.float32, device=given.device) if want_bias else None
    partials = None
    if want_bias or (vector and g_std is not None):
        needed = _native.lib().cusrl_symmetric_head_num_partials(B, A)
        partials = torch.empty(max(int(needed), 1), dtype=torch.float64, device=given.device)
    _checked.cusrl_symmetric_head_bwd(_ptr(g_mean), _ptr(g_std), std2.data_ptr(), int(vector), table.data_ptr(), B, A,
            _ptr(d_mean2), _ptr(d_std2), _ptr(d_bias), _ptr(partials), _stream())
    if B == 0:  # (no rows: the launch is a no-op, the column sums are empty)
        if vector and d_std2 is not None:
            d_std2.zero_()
        if d_bias is not None:
            d_bias.zero_()
    return d_mean2, d_std2, d_bias
