"""Observation hooks (counterparts of cusrl/hook/mdp/observation.py): ``ObservationNanToNum`` (17-56) and the online
observation / state normalisation ``ObservationNormalization`` (59-255).

``ObservationNanToNum`` replaces NaN / +Inf / -Inf in the incoming tensors in place — ``observation`` and ``state`` in
``pre_act``, ``next_observation`` and ``next_state`` in ``post_step`` — as ONE HIP launch per hook call
(``cusrl_nan_to_num2`` takes both tensors), which reads every element and writes only the 16-byte lanes it changed.

``pre_act`` and ``post_step`` update running statistics with the incoming (next) observation and replace it by its
normalised, clamped value, keeping the raw tensors under ``original_*`` (they become extra buffer leaves and ride
the same push / gather launches).  On MI355X an update is masked column statistics + merge + normalise = three HIP
launches with the sample count kept on the device; the reference's ``observation[last_done]`` boolean-mask select
(observation.py:206-208), which synchronises with the host every step, becomes the kernel's row mask.  With
``mirror_observation`` / ``mirror_state`` in the spec the batch statistics are made symmetric before the merge
(observation.py:213-217): one more launch (``cusrl_symmetrize_mean_var``) for a ``MirrorDef``; any other mirror callable is
evaluated as given on the ``[C]`` statistics.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from cusrl_amd import ops
from cusrl_amd.hook.auxiliary.symmetry import MirrorDef
from cusrl_amd.nn.rms import RunningMeanStd, mean_var_count
from cusrl_amd.template.hook import Hook
from cusrl_amd.utils.misc import host_form

__all__ = ["ObservationNanToNum", "ObservationNormalization"]


def _symmetric(stats, mirror):
    """observation.py:213-217: the batch statistics of the mirrored data merged with the original's, before the merge into
    the running statistics (and before any cross-rank merge)."""
    mean, var, count = stats
    if mirror is None:
        return stats
    if isinstance(mirror, MirrorDef) and mean.is_cuda:
        mean, var = mean.float().contiguous(), var.float().contiguous()
        ops.symmetrize_mean_var_(mean, var, mirror.device_table(mean.device, mean.numel()))
        return mean, var, count
    if not mean.is_cuda:  # (a user-supplied mirror callable on the device is evaluated as given)
        host_form("ObservationNormalization (symmetric statistics)")
    mirrored_mean = mirror(mean)
    mirrored_var = abs(mirror(var))
    var = (var + mirrored_var) / 2 + (mean - mirrored_mean) ** 2 / 4
    mean = (mean + mirrored_mean) / 2
    return mean, var, count


class ObservationNanToNum(Hook):
    """``tensor.nan_to_num_(nan=, posinf=, neginf=)`` on whatever of the four fields is present (missing or None: skipped)."""

    # nothing random, no Python state per step: an env step with this hook may be replayed from a hipGraph.  Its post_step
    # WRITES the transition on the device, so `post_step_device_free` stays False (the default of an overriding hook): the
    # captured step keeps the step epilogue and the append as separate launches around it.
    rollout_capture_safe = True

    def __init__(self, nan: float = 0.0, posinf: float = 0.0, neginf: float = 0.0):
        super().__init__()
        self.nan = nan
        self.posinf = posinf
        self.neginf = neginf

    def nan_to_num_(self, tensor: Tensor | None):
        self._sanitize(tensor, None)

    def pre_act(self, transition):
        self._sanitize(transition.get("observation"), transition.get("state"))

    def post_step(self, transition):
        self._sanitize(transition.get("next_observation"), transition.get("next_state"))

    def export_stages(self, which: str = "actor"):
        return (({"kind": "nan_to_num", "nan": float(self.nan), "posinf": float(self.posinf), "neginf": float(self.neginf)}, {}),)

    def _sanitize(self, first: Tensor | None, second: Tensor | None):
        tensors = [t for t in (first, second) if t is not None]
        if not tensors:
            return
        if not all(isinstance(t, Tensor) and t.is_cuda for t in tensors):
            host_form("ObservationNanToNum")  # test processes without a GPU only
            for t in tensors:
                t.nan_to_num_(nan=self.nan, posinf=self.posinf, neginf=self.neginf)
            return
        direct, staged = [], []
        for t in tensors:
            if t.dtype == torch.float32 and t.is_contiguous():
                direct.append(t)
            elif t.dtype in (torch.float32, torch.float16, torch.bfloat16):
                # a layout / width the launch does not take goes through a contiguous fp32 copy (exact: every fp16 / bf16
                # value, NaN payloads' class and the infinities included, is an fp32 value) and back
                staged.append((t, t.float().contiguous()))
            else:
                # float64, integers, bool: the ONE place a torch element-wise op is acceptable — an fp32 copy would round a
                # float64 observation, and on integers / bool the operation changes nothing
                t.nan_to_num_(nan=self.nan, posinf=self.posinf, neginf=self.neginf)
        work = direct + [copy for _, copy in staged]
        for i in range(0, len(work), 2):  # both fields of a call in one launch
            ops.nan_to_num_(work[i], work[i + 1] if i + 1 < len(work) else None, nan=self.nan, posinf=self.posinf,
                            neginf=self.neginf)
        for t, copy in staged:
            t.copy_(copy)


class ObservationNormalization(Hook):
    def __init__(self, max_count: int | None = None, defer_synchronization: bool = False, renormalize: bool = False):
        if max_count is not None and max_count <= 0:
            raise ValueError("'max_count' must be positive or None")
        super().__init__()
        self.max_count = max_count
        self.defer_synchronization = defer_synchronization
        self.renormalize = renormalize
        self.frozen: bool = False
        self.register_mutable("frozen")
        self.observation_rms: RunningMeanStd
        self.state_rms: RunningMeanStd | None = None
        self._observation_is_subset_of_state = None
        self._mirror_observation = None
        self._mirror_state = None
        self._last_done: Tensor | None = None

    def freeze(self):
        self.frozen = True
        return self

    def init(self):
        spec = self.agent.environment_spec
        self._mirror_observation = spec.mirror_observation
        self._mirror_state = spec.mirror_state
        device = getattr(self.agent, "device", None)
        if device is not None and torch.device(device).type == "cuda":  # tables uploaded now, outside any capture
            mirrors = [(self._mirror_observation, self.agent.observation_dim)]
            if self.agent.has_state:  # (without a state the agent's state_dim is the observation's; a state mirror is unused)
                mirrors.append((self._mirror_state, self.agent.state_dim))
            for mirror, dim in mirrors:
                if isinstance(mirror, MirrorDef):
                    mirror.device_table(device, dim)
        subset = spec.observation_is_subset_of_state
        if subset is not None:
            if not self.agent.has_state:
                raise ValueError("'observation_is_subset_of_state' is set without defining the state")
            if isinstance(subset, (np.ndarray, list, tuple)):
                subset = self.agent.to_tensor(np.asarray(subset))
            self._observation_is_subset_of_state = subset
            self.register_module("observation_rms", RunningMeanStd(self.agent.observation_dim))
        else:
            self.register_module("observation_rms", RunningMeanStd(
                self.agent.observation_dim, max_count=self.max_count, groups=spec.observation_stat_groups,
                excluded_indices=spec.observation_normalization_excluded_indices))
        if self.agent.has_state:
            self.register_module("state_rms", RunningMeanStd(
                self.agent.state_dim, max_count=self.max_count, groups=spec.state_stat_groups,
                excluded_indices=spec.state_normalization_excluded_indices))
        else:
            self.state_rms = None

    def collective_phases(self):
        # every statistics update all-gathers (mean, var, count) unless synchronisation is deferred to pre_update
        return () if (self.defer_synchronization or self.frozen) else ("act",)

    def on_replay(self, phase):
        # a replayed statistics update happened on the device only: the modules' "synchronised" flags are host state
        if self.defer_synchronization and not (self.frozen or self.agent.inference_mode):
            for rms in (self.observation_rms, self.state_rms):
                if rms is not None:
                    rms._is_synchronized = False

    # ---- rollout
    def pre_act(self, transition):
        observation, state = transition["observation"], transition.get("state")
        if self._last_done is None:
            # persistent mask buffer (all rows on the very first step): a fixed address keeps pre_act capturable
            # into the act hipGraph, post_step refreshes its contents in place
            self._last_done = torch.ones(observation.shape[0], dtype=torch.bool, device=observation.device)
            self._update_rms(observation, state, self._last_done)
        elif not self.agent.environment_spec.final_state_is_missing:
            # after the first step only freshly reset envs carry an observation the statistics have not seen yet
            self._update_rms(observation, state, self._last_done)
        transition["original_observation"] = observation
        transition["observation"] = self.observation_rms.normalize(observation)
        if self.state_rms is not None:
            transition["original_state"] = state
            transition["state"] = self.state_rms.normalize(state)

    def post_step(self, transition):
        next_observation, next_state = transition["next_observation"], transition.get("next_state")
        self._update_rms(next_observation, next_state)
        done = transition["done"].squeeze(-1)
        if self._last_done is None or self._last_done.shape != done.shape:
            self._last_done = done.clone()
        else:
            self._last_done.copy_(done)
        transition["original_next_observation"] = next_observation
        transition["next_observation"] = self.observation_rms.normalize(next_observation)
        if self.state_rms is not None:
            transition["original_next_state"] = next_state
            transition["next_state"] = self.state_rms.normalize(next_state)

    def _update_rms(self, observation: Tensor, state: Tensor | None, mask: Tensor | None = None):
        if self.agent.inference_mode or self.frozen:
            return
        synchronize = not self.defer_synchronization
        if state is not None:
            self.state_rms.update_from_stats(*_symmetric(mean_var_count(state, mask), self._mirror_state), synchronize=synchronize)
        if self._observation_is_subset_of_state is not None:
            self._copy_observation_stats_from_state()
        else:
            self.observation_rms.update_from_stats(*_symmetric(mean_var_count(observation, mask), self._mirror_observation),
                                                   synchronize=synchronize)

    def _copy_observation_stats_from_state(self):
        index = self._observation_is_subset_of_state
        self.observation_rms.mean.copy_(self.state_rms.mean[index])
        self.observation_rms.var.copy_(self.state_rms.var[index])
        self.observation_rms.std.copy_(self.state_rms.std[index])
        self.observation_rms._count.copy_(self.state_rms._count)

    def export_stages(self, which: str = "actor"):
        """The actor sees observations, so its stage carries the OBSERVATION statistics (never the state's), as they stand."""
        rms = self.observation_rms
        return (({"kind": "normalize", "clamp": rms.clamp, "epsilon": float(rms.epsilon)}, {"mean": rms.mean, "std": rms.std}),)

    # ---- update
    def pre_update(self, buffer):
        if self.defer_synchronization:
            if self.state_rms is not None:
                self.state_rms.synchronize()
            if self._observation_is_subset_of_state is not None:
                self._copy_observation_stats_from_state()
            else:
                self.observation_rms.synchronize()

    def objective(self, metadata, batch):
        if self.renormalize:
            batch["observation"] = self.observation_rms.normalize(batch["original_observation"])
            batch["next_observation"] = self.observation_rms.normalize(batch["original_next_observation"])
            if self.state_rms is not None:
                batch["state"] = self.state_rms.normalize(batch["original_state"])
                batch["next_state"] = self.state_rms.normalize(batch["original_next_state"])
