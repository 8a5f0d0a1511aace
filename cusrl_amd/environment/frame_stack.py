"""``FrameStack``: an environment whose observation is the last ``stack_size`` observations of the environment it wraps, oldest
first (gymnasium's ``FrameStackObservation(env, stack_size, padding_type)``; ``csrc/frame_stack.hip``; DESIGN.md §7, "Frame
stacking").

The history ``[N, S, K]`` lives in HBM beside the inner env's state.  ``step`` is the inner step and ONE ``cusrl_frame_stack_push``
launch, ``reset`` / ``reset_static`` the inner reset and ONE ``cusrl_frame_stack_reset`` launch; nothing is read by the host and
no Python state changes per step, so the wrapper is ``capturable`` / ``generator_free`` exactly when the inner env is and a
wrapped task still replays its whole rollout from one hipGraph.  On CPU tensors the same calls run the library's host
restatements of the two kernels (behind ``utils.misc.host_form``)."""

from __future__ import annotations

import torch

from cusrl_amd.template.environment import _SPEC_DEFAULTS, Environment

__all__ = ["FrameStack"]

# Spec properties that describe the layout of the INNER observation: an index list, a normaliser or a mirror definition over K0
# columns means something else over S * K stacked ones, and the wrapper does not guess the translation.
_OBSERVATION_BOUND = ("mirror_observation", "observation_is_subset_of_state", "observation_normalization",
                      "observation_normalization_excluded_indices", "observation_space", "observation_stat_groups")
_OWN = ("observation_dim", "action_dim", "device", "environment_instance")


class FrameStack(Environment):
    """``FrameStack(env, stack_size, padding_type="reset", columns=None)`` around any :class:`Environment` of this package whose
    observations are contiguous fp32 ``[N, K0]`` tensors.  ``columns`` (distinct indices into ``K0``) selects and orders the
    columns that are kept: ``K = len(columns)``; ``spec.observation_dim = stack_size * K``.  The privileged state, the reward,
    both flags, the info dict, ``get_metrics``, ``state_dict`` and ``close`` are the inner env's, untouched.  The stacked row of
    an env that finished carries its terminal observation as the newest slot — what bootstrapping on truncation reads; the env's
    next history starts from its reset observation by ``padding_type`` (``"reset"``: repeated in every slot; ``"zero"``: zeros in
    front of it)."""

    def __init__(self, env: Environment, stack_size: int, padding_type: str = "reset", columns=None):
        from cusrl_amd import ops

        if not isinstance(env, Environment):
            raise TypeError(f"FrameStack wraps an Environment of this package; got {type(env).__name__}")
        self.stack_size = int(stack_size)
        if self.stack_size < 1:
            raise ValueError(f"stack_size must be at least 1; got {stack_size}")
        ops.frame_stack_padding(padding_type)
        spec = env.spec
        def declared(value) -> bool:
            return value is not None and not (isinstance(value, (tuple, list)) and len(value) == 0)

        untranslatable = [name for name in _OBSERVATION_BOUND if declared(spec.get(name, _SPEC_DEFAULTS[name]))]
        if spec.autoreset:
            untranslatable.append("autoreset")  # (the inner env would restart inside its step, where the wrapper cannot see it)
        if untranslatable:
            raise ValueError(f"FrameStack cannot translate the inner environment's spec propert{'ies' if len(untranslatable) > 1 else 'y'} "
                             f"{', '.join(untranslatable)} to the stacked observation; wrap an environment without "
                             f"{'them' if len(untranslatable) > 1 else 'it'} and declare {'them' if len(untranslatable) > 1 else 'it'} "
                             "over the stacked layout")
        device = spec.device
        self.env, self.device, self.padding_type = env, device, padding_type
        self._columns = ops.frame_stack_columns(columns, env.observation_dim, device)
        self.columns = None if self._columns is None else tuple(self._columns.tolist())
        self.width = env.observation_dim if self.columns is None else len(self.columns)
        carried = {name: value for name, value in spec.__dict__.items() if name not in _OBSERVATION_BOUND and name not in _OWN}
        num_instances, state_dim = carried.pop("num_instances"), carried.pop("state_dim")
        super().__init__(self.stack_size * self.width, env.action_dim, num_instances=num_instances, state_dim=state_dim, device=device,
                         **carried)
        self.capturable = bool(getattr(env, "capturable", False))
        self.generator_free = bool(getattr(env, "generator_free", False))
        # (allocated once and only ever written in place: captured steps hold its address)
        self.history = torch.zeros(num_instances, self.stack_size, self.width, dtype=torch.float32, device=device)
        self._all = torch.arange(num_instances, dtype=torch.int64, device=device)

    def _ops(self):
        """``(push, reset)``: the kernels for a device history, the library's host restatements behind the gate otherwise."""
        from cusrl_amd import ops

        if self.history.is_cuda:
            return ops.frame_stack_push, ops.frame_stack_reset
        from cusrl_amd.utils.misc import host_form

        host_form("FrameStack")
        return ops.frame_stack_push_cpu, ops.frame_stack_reset_cpu

    def reset(self, *, indices=None, randomize_episode_progress: bool = False):
        observation, state, info = self.env.reset(indices=indices, randomize_episode_progress=randomize_episode_progress)
        if indices is None:
            indices = self._all
        else:
            indices = torch.as_tensor(indices, dtype=torch.int64, device=self.device).reshape(-1).contiguous()
        stacked = self._ops()[1](self.history, indices, None, observation, self._columns, self.padding_type)
        return stacked, state, info

    def reset_static(self, indices, count):
        observation, state, info = self.env.reset_static(indices, count)
        stacked = self._ops()[1](self.history, indices, count, observation, self._columns, self.padding_type)
        return stacked, state, info

    def step(self, action):
        next_observation, next_state, reward, terminated, truncated, info = self.env.step(action)
        stacked = self._ops()[0](self.history, next_observation, self._columns, None, self.padding_type)
        return stacked, next_state, reward, terminated, truncated, info

    def close(self):
        self.env.close()

    def get_metrics(self):
        return self.env.get_metrics()

    def state_dict(self):
        return self.env.state_dict()

    def load_state_dict(self, state_dict):
        """The inner env's checkpoint; the history is not part of it: call ``reset`` before stepping a loaded env."""
        self.env.load_state_dict(state_dict)
