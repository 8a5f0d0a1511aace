"""Reward hooks.  ``RewardShaping``: affine reward shaping with optional clamping (counterpart of cusrl/hook/mdp/reward.py:10-47),
on a GPU one HIP launch (``cusrl_reward_shaping``) for the reference's ``mul_`` / ``add_`` / ``clamp_`` chain.
``RewardNormalization``: rewards divided by the running standard deviation of the discounted return (gymnasium's
``NormalizeReward``, SB3's ``VecNormalize(norm_reward=True)``; the reference has no counterpart), on a GPU one HIP launch per env
step (``cusrl_reward_normalize``)."""

from __future__ import annotations

import torch
from torch import nn

from cusrl_amd.nn.rms import _synchronize_mean_var_count, merge_mean_var_
from cusrl_amd.template.hook import Hook
from cusrl_amd.utils import distributed
from cusrl_amd.utils.misc import host_form

__all__ = ["RewardNormalization", "RewardShaping"]


class RewardShaping(Hook):
    def __init__(self, scale: float = 1.0, shift: float = 0.0, lower_bound: float | None = None, upper_bound: float | None = None):
        super().__init__()
        self.scale, self.shift, self.lower_bound, self.upper_bound = scale, shift, lower_bound, upper_bound

    def post_step(self, transition):
        reward = transition["reward"]
        bounded = self.lower_bound is not None or self.upper_bound is not None
        if self.scale == 1.0 and self.shift == 0.0 and not bounded:
            return  # the identity: nothing to launch
        if isinstance(reward, torch.Tensor) and reward.is_cuda:
            from cusrl_amd import ops

            if reward.dtype == torch.float32 and reward.is_contiguous():
                ops.reward_shaping_(reward, self.scale, self.shift, self.lower_bound, self.upper_bound)
            else:  # a layout the launch does not take is staged, not handed to torch's elementwise ops
                staged = reward.float().contiguous()
                ops.reward_shaping_(staged, self.scale, self.shift, self.lower_bound, self.upper_bound)
                reward.copy_(staged)
            return
        host_form("RewardShaping.post_step")  # test processes without a GPU only
        reward.mul_(self.scale).add_(self.shift)
        if bounded:
            reward.clamp_(min=self.lower_bound, max=self.upper_bound)


class ReturnStatistics(nn.Module):
    """The device state of :class:`RewardNormalization`: ``returns [N, R]`` fp32, the discounted return per env and reward column,
    and ``stats [3, R]`` float64, the rows running mean, variance and count of the returns (gymnasium's ``RunningMeanStd`` start:
    0, 1, 1e-4).  Allocated once; ``load_state_dict`` copies into the same storage, so a captured step keeps its addresses."""

    def __init__(self, num_instances: int, reward_dim: int):
        super().__init__()
        self.register_buffer("returns", torch.zeros(num_instances, reward_dim, dtype=torch.float32))
        stats = torch.zeros(3, reward_dim, dtype=torch.float64)
        stats[1] = 1.0
        stats[2] = 1e-4
        self.register_buffer("stats", stats)

    @property
    def mean(self) -> torch.Tensor:
        return self.stats[0]

    @property
    def var(self) -> torch.Tensor:
        return self.stats[1]

    @property
    def count(self) -> torch.Tensor:
        return self.stats[2]


class RewardNormalization(Hook):
    """``reward / sqrt(var + epsilon)`` in ``post_step``, ``var`` the running variance of the discounted return
    ``G <- G * gamma + reward`` over every env and step so far; the mean is not subtracted; ``clip``: the result clamped to
    ``±clip``; the return of an env that terminated or was truncated starts again from 0.  ``update=False`` freezes the statistics
    (an agent in inference mode never updates them).  One launch per env step does all of it; order of the operations, precisions
    and the summation order: include/cusrl_hip.h, ``cusrl_reward_normalize``.

    Non-finite rewards are NOT filtered: a NaN or Inf reward enters the return and the statistics of its column, after which every
    normalised reward of that column is non-finite.  A task that can emit them puts ``RewardShaping`` bounds in front.

    The trainer's episode statistics are taken before the agent's hooks run: the logged episode return is the raw reward, as with
    ``RewardShaping``.  The buffer, and so the value targets, hold the normalised reward.

    Several ranks: the step is rank-local; the ranks' statistics are merged in ``pre_update``, the point at which
    ``ObservationNormalization(defer_synchronization=True)`` merges its own, with the same helper (what each rank added since the
    last merge, pooled by count)."""

    rollout_capture_safe = True  # no random draws, no host read, no Python state per step beyond a flag repeated in on_replay

    def __init__(self, gamma: float = 0.99, epsilon: float = 1e-8, clip: float | None = None, update: bool = True):
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("'gamma' must be within [0, 1]")
        if epsilon < 0:
            raise ValueError("'epsilon' must be non-negative")
        if clip is not None and not clip >= 0:
            raise ValueError("'clip' must be None or non-negative")
        super().__init__()
        for name, value in (("gamma", gamma), ("epsilon", epsilon), ("clip", clip), ("update", update)):
            self.register_mutable(name, value)  # host arguments of the launch: a change re-captures the step
        self.statistics: ReturnStatistics
        self._is_synchronized = True
        self._synchronized_state: tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None = None

    def init(self):
        self.register_module("statistics", ReturnStatistics(self.agent.parallelism, self.agent.environment_spec.reward_dim))

    def _updating(self) -> bool:
        return bool(self.update) and not self.agent.inference_mode

    def post_step(self, transition):
        from cusrl_amd import ops

        reward, statistics = transition["reward"], self.statistics
        direct = reward.dtype == torch.float32 and reward.is_contiguous()
        staged = reward if direct else reward.float().contiguous()  # a layout the launch does not take goes through a copy
        ops.reward_normalize_(staged, statistics.returns, transition["terminated"], transition["truncated"], statistics.stats,
                              self.gamma, self.epsilon, self.clip, self._updating())
        if not direct:
            reward.copy_(staged)
        if self._updating():
            self._is_synchronized = False

    def on_replay(self, phase):
        if phase == "step" and self._updating():  # the launch was replayed; the flag is host state
            self._is_synchronized = False

    # ---- several ranks
    def pre_update(self, buffer):
        self.synchronize()

    def synchronize(self):
        """Merge what every rank added since the last merge (``RunningMeanStd.synchronize``, over the float64 triple).  The count is
        one number: every column has seen the same rows."""
        if self._is_synchronized or not distributed.enabled():
            return
        statistics = self.statistics
        mean, var, count = statistics.mean, statistics.var, statistics.count[:1]
        if self._synchronized_state is None:
            total_mean, total_var, total_count = _synchronize_mean_var_count(mean, var, count)
        else:
            sync_mean, sync_var, sync_count = self._synchronized_state
            local, base = float(count.item()), float(sync_count.item())
            merge_mean_var_(mean, var, local, sync_mean, sync_var, -base)  # what this rank added since
            patch = _synchronize_mean_var_count(mean, var, count - sync_count)
            merge_mean_var_(sync_mean, sync_var, base, patch[0], patch[1], float(patch[2].item()))
            total_mean, total_var, total_count = sync_mean, sync_var, sync_count + patch[2]
        mean.copy_(total_mean)
        var.copy_(total_var)
        statistics.count.copy_(total_count.expand_as(statistics.count))
        self._mark_synchronized()

    def _mark_synchronized(self):
        statistics = self.statistics
        self._is_synchronized = True
        self._synchronized_state = (statistics.mean.clone(), statistics.var.clone(), statistics.count[:1].clone())

    # ---- checkpoint: the device state and the hyper-parameters
    def state_dict(self):
        state = super().state_dict()
        state["hyper_parameters"] = {"gamma": self.gamma, "epsilon": self.epsilon, "clip": self.clip, "update": self.update}
        return state

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        for name, value in (state_dict.pop("hyper_parameters", None) or {}).items():
            self.update_attribute(name, value)
        super().load_state_dict(state_dict)
        self._mark_synchronized()
