"""Reward normalisation (``csrc/reward_norm.hip``): the discounted return per env, its running statistics and the rescaled
reward in ONE launch.  Formulas, summation order and argument rules: include/cusrl_hip.h.  Device tensors go to the kernel; CPU
tensors go to the library's host restatement (``cusrl_reward_normalize_cpu``, the same ``__host__ __device__`` bodies in the
kernel's summation order) behind the ``host_form`` gate — the hook's host form and what the GPU tests compare the kernel against."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd._native import check
from cusrl_amd.ops._common import _checked, _modified_in_place, _stream
from cusrl_amd.utils.misc import host_form

__all__ = ["reward_normalize_", "reward_normalize_cpu_"]


def _describe(value) -> str:
    if not isinstance(value, torch.Tensor):
        return type(value).__name__
    return f"{value.dtype} {tuple(value.shape)} on {value.device}{'' if value.is_contiguous() else ' (strided)'}"


def reward_normalize_(reward: torch.Tensor, returns: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor,
                      stats: torch.Tensor, gamma: float, epsilon: float, clip: float | None = None, update: bool = True, *,
                      _host: bool = False) -> torch.Tensor:
    """``cusrl_reward_normalize``, ONE launch, everything in place: ``returns [N, R]`` becomes ``returns * gamma + reward``; with
    ``update`` its batch mean, population variance and count are merged into ``stats [3, R]`` (float64 rows mean, var, count);
    ``reward [N, R]`` is divided by ``sqrt(var + epsilon)`` and clamped to ``±clip``; the returns of the envs with
    ``terminated | truncated`` (``[N]`` or ``[N, 1]`` bool) are zeroed.  Returns ``reward``.  CPU tensors: the host restatement."""
    ok = (isinstance(reward, torch.Tensor) and reward.dtype == torch.float32 and reward.dim() == 2 and reward.shape[1] >= 1
          and reward.is_contiguous())
    if not ok:
        raise ValueError(f"reward_normalize_: 'reward' must be a contiguous float32 [N, R] tensor; got {_describe(reward)}")
    N, R = reward.shape
    device = reward.device
    if not (isinstance(returns, torch.Tensor) and returns.dtype == torch.float32 and returns.shape == reward.shape
            and returns.device == device and returns.is_contiguous()):
        raise ValueError(f"reward_normalize_: 'returns' must be a contiguous float32 [{N}, {R}] tensor on {device}; got {_describe(returns)}")
    for name, flags in (("terminated", terminated), ("truncated", truncated)):
        if not (isinstance(flags, torch.Tensor) and flags.dtype in (torch.bool, torch.uint8) and flags.numel() == N
                and flags.dim() in (1, 2) and flags.shape[0] == N and flags.device == device and flags.is_contiguous()):
            raise ValueError(f"reward_normalize_: '{name}' must be a contiguous bool [{N}] or [{N}, 1] tensor on {device}; got {_describe(flags)}")
    if not (isinstance(stats, torch.Tensor) and stats.dtype == torch.float64 and stats.shape == (3, R) and stats.device == device
            and stats.is_contiguous()):
        raise ValueError(f"reward_normalize_: 'stats' must be a contiguous float64 [3, {R}] tensor on {device}; got {_describe(stats)}")
    if clip is not None and not clip >= 0:
        raise ValueError(f"reward_normalize_: 'clip' must be None or non-negative; got {clip}")
    arguments = (reward.data_ptr(), returns.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), stats.data_ptr(), float(gamma),
                 float(epsilon), 0.0 if clip is None else float(clip), int(clip is not None), int(bool(update)), N, R)
    if reward.is_cuda:
        _checked.cusrl_reward_normalize(*arguments, _stream())
    else:
        if not _host:
            host_form("reward_normalize_")
        check(_native.lib().cusrl_reward_normalize_cpu(*arguments), "cusrl_reward_normalize_cpu")
    _modified_in_place(reward)
    _modified_in_place(returns)
    if update:
        _modified_in_place(stats)
    return reward


def reward_normalize_cpu_(reward, returns, terminated, truncated, stats, gamma: float, epsilon: float, clip: float | None = None,
                          update: bool = True) -> torch.Tensor:
    """:func:`reward_normalize_` by the library's host restatement, over CPU tensors (no ``host_form`` gate: asked for by name)."""
    if not (isinstance(reward, torch.Tensor) and not reward.is_cuda):
        raise ValueError(f"reward_normalize_cpu_: 'reward' must be a CPU tensor; got {_describe(reward)}")
    return reward_normalize_(reward, returns, terminated, truncated, stats, gamma, epsilon, clip, update, _host=True)
