"""Value targets, GAE and the advantage statistics / normalisation (``csrc/advantage.hip``)."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _f32, _flag, _modified_in_place, _observed, _ptr, _stream, require_device


def next_value(
    value: torch.Tensor,
    terminated: torch.Tensor,
    truncated: torch.Tensor,
    last_value: torch.Tensor,
    termination_value: float,
    truncated_uses_own_value: bool,
    out: torch.Tensor,
) -> torch.Tensor:
    """Bootstrap target of cusrl/hook/on_policy/value.py:66-70,79-80; returns the per-block truncated counters."""
    value = _f32(value, "value")
    T, N, D = value.shape
    terminated, truncated = _flag(terminated, "terminated"), _flag(truncated, "truncated")
    last_value = _f32(last_value, "last_value")
    if last_value.numel() != N * D or out.shape != value.shape or not out.is_contiguous():
        raise ValueError("next_value: inconsistent shapes")
    lib = _native.lib()
    block_counts = torch.empty(max(int(lib.cusrl_flag_blocks(T * N)), 1), dtype=torch.int32, device=value.device)
    out_ptr = _f32(out, "next_value").data_ptr()
    _observed("cusrl_next_value", value.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), last_value.data_ptr(),
            float(termination_value), int(truncated_uses_own_value), out_ptr, block_counts.data_ptr(), T, N, D,
            nbytes=lambda: T * N * (8 * D + 2))
    return block_counts


def gae(
    reward: torch.Tensor,
    value: torch.Tensor,
    next_value_: torch.Tensor,
    done: torch.Tensor,
    gamma: float,
    lamda: float,
    lamda_value: float | None,
    advantage: torch.Tensor | None = None,
    ret: torch.Tensor | None = None,
    with_stats: bool = True,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None]:
    """Fused delta + backward scan + return (+ advantage {sum, sumsq} partials) — gae.py:8-20, 85-110."""
    reward, value, next_value_ = _f32(reward, "reward"), _f32(value, "value"), _f32(next_value_, "next_value")
    done = _flag(done, "done")
    if reward.dim() < 2 or reward.shape != value.shape or reward.shape != next_value_.shape:
        raise ValueError(f"gae: reward/value/next_value shapes differ: {reward.shape}, {value.shape}, {next_value_.shape}")
    T, N = reward.shape[:2]
    D = reward.numel() // max(T * N, 1)
    if done.numel() != T * N:
        raise ValueError(f"gae: 'done' must be [T, N, 1]; got {tuple(done.shape)}")
    for out, name in ((advantage, "advantage"), (ret, "return")):
        if out is not None and (not out.is_contiguous() or out.shape != reward.shape):
            raise ValueError(f"gae: the '{name}' output must be a contiguous tensor of the reward's shape (results are "
                             "written in place; a strided view would silently receive nothing)")
    advantage = torch.empty_like(reward) if advantage is None else _f32(advantage, "advantage")
    ret = torch.empty_like(reward) if ret is None else _f32(ret, "return")
    lib = _native.lib()
    partials = None
    if with_stats:
        partials = torch.empty((max(int(lib.cusrl_gae_num_partials(T, N, D)), 1), D, 2), dtype=torch.float64, device=reward.device)
    _observed("cusrl_gae", reward.data_ptr(), value.data_ptr(), next_value_.data_ptr(), done.data_ptr(), advantage.data_ptr(),
            ret.data_ptr(), _ptr(partials), T, N, D, float(gamma), float(lamda), -1.0 if lamda_value is None else float(lamda_value),
            nbytes=lambda: T * N * (20 * D + 1))
    return advantage, ret, partials


def col_stats(x: torch.Tensor) -> torch.Tensor:
    """Per-channel {sum, sumsq} partials of ``x [..., D]`` (first pass of advantage.py:111)."""
    x = _f32(x, "x")
    D = x.shape[-1]
    rows = x.numel() // max(D, 1)
    lib = _native.lib()
    partials = torch.empty((max(int(lib.cusrl_col_stats_num_partials(rows, D)), 1), D, 2), dtype=torch.float64, device=x.device)
    _checked.cusrl_col_stats(x.data_ptr(), rows, D, partials.data_ptr(), _stream())
    return partials


def adv_stats_finalize(partials: torch.Tensor, count: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``var, mean`` (unbiased) from block partials, fixed summation order.  The two are the halves of ONE ``[2 D]`` row
    (``mean | var`` — what a cross-rank merge gathers: ``packed_mean_var`` hands it over without a ``torch.cat``)."""
    P, D, _ = partials.shape
    row = torch.empty(2 * D, dtype=torch.float32, device=partials.device)
    mean, var = row[:D], row[D:]
    _checked.cusrl_stats_finalize(partials.data_ptr(), P, D, count, mean.data_ptr(), var.data_ptr(), _stream())
    return var, mean


def normalize_(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """``x.sub_(mean).div_((var + eps).sqrt())`` in place (advantage.py:114-115)."""
    require_device(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("normalize_: expected a contiguous float32 tensor")
    D = x.shape[-1]
    mean, var = _f32(mean, "mean"), _f32(var, "var")
    _observed("cusrl_normalize", x.data_ptr(), mean.data_ptr(), var.data_ptr(), eps, x.numel() // max(D, 1), D,
            nbytes=lambda: x.numel() * 8)
    _modified_in_place(x)
    return x


def normalize_from_partials_(x: torch.Tensor, partials: torch.Tensor, count: int, eps: float = 1e-8) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`adv_stats_finalize` + :func:`normalize_` as ONE launch (single-process case); returns ``(var, mean)``."""
    require_device(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("normalize_from_partials_: expected a contiguous float32 tensor")
    P, D, _ = partials.shape
    if x.shape[-1] != D:
        raise ValueError("normalize_from_partials_: the partials belong to another tensor")
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    var = torch.empty(D, dtype=torch.float32, device=x.device)
    _observed("cusrl_normalize_from_partials", x.data_ptr(), partials.data_ptr(), P, count, eps, x.numel() // max(D, 1), D,
            mean.data_ptr(), var.data_ptr(), nbytes=lambda: x.numel() * 8)
    _modified_in_place(x)
    return var, mean


def packed_mean_var(mean: torch.Tensor, var: torch.Tensor) -> torch.Tensor:
    """``[mean | var]`` as one contiguous row: the halves of :func:`adv_stats_finalize`'s row as they are (no launch), else a
    ``torch.cat``."""
    D = mean.numel()
    if (mean.dim() == var.dim() == 1 and var.numel() == D and mean.is_contiguous() and var.is_contiguous()
            and mean.untyped_storage().data_ptr() == var.untyped_storage().data_ptr()
            and var.storage_offset() == mean.storage_offset() + D):
        return mean.as_strided((2 * D,), (1,), mean.storage_offset())
    return torch.cat((mean, var), dim=0)


def normalize_from_gathered_(x: torch.Tensor, gathered: torch.Tensor, eps: float = 1e-8) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`merge_mean_var` + :func:`normalize_` as ONE launch: ``gathered [W, 2 D]`` holds every rank's ``mean | var``;
    returns the merged ``(var, mean)``."""
    require_device(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("normalize_from_gathered_: expected a contiguous float32 tensor")
    gathered = _f32(gathered, "gathered")
    D = x.shape[-1]
    if gathered.dim() != 2 or gathered.shape[1] != 2 * D:
        raise ValueError("normalize_from_gathered_: expected [W, 2 D] rows of mean | var")
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    var = torch.empty(D, dtype=torch.float32, device=x.device)
    _observed("cusrl_normalize_from_gathered", x.data_ptr(), gathered.data_ptr(), gathered.shape[0], eps, x.numel() // max(D, 1), D,
            mean.data_ptr(), var.data_ptr(), nbytes=lambda: x.numel() * 8)
    _modified_in_place(x)
    return var, mean


def merge_mean_var(gathered: torch.Tensor, mean: torch.Tensor, var: torch.Tensor) -> None:
    """Equal-weight cross-rank merge of distributed.py:175-183 from the all-gathered ``[W, 2D]`` rows."""
    gathered = _f32(gathered, "gathered")
    W, twoD = gathered.shape
    _checked.cusrl_merge_mean_var(gathered.data_ptr(), W, twoD // 2, _f32(mean, "mean").data_ptr(), _f32(var, "var").data_ptr(), _stream())
