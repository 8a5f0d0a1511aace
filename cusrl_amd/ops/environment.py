"""The classic-control tasks (``csrc/environment.hip``): one launch per env step, one per reset.  Formulas, constants and argument
rules: include/cusrl_hip.h.  Device tensors go to the kernels; CPU tensors go to the library's host restatements (``*_cpu``, the
same ``__host__ __device__`` bodies) behind the ``host_form`` gate — the host form of the environments and what the GPU tests
compare the kernels against."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd._native import check
from cusrl_amd.ops._common import _checked, _modified_in_place, _ptr, _stream
from cusrl_amd.utils.misc import host_form

__all__ = ["CLASSIC_TASKS", "ClassicTask", "classic_reset", "classic_reset_cpu", "classic_step", "classic_step_cpu"]


class ClassicTask:
    """One task's code and row widths (``CUSRL_CLASSIC_*`` of the header; the widths as in the task's ``Task<kind>`` block of the kernel file,
    which also holds its formulas)."""

    def __init__(self, name: str, constant: str, state_dim: int, action_dim: int, observation_dim: int, max_episode_steps: int):
        self.name, self.kind = name, _native._CONSTANTS[constant]
        self.state_dim, self.action_dim, self.observation_dim = state_dim, action_dim, observation_dim
        self.max_episode_steps = max_episode_steps


# The two later tasks are keyed by their gym ids ONLY: the bare name "Acrobot" is the suite's standing example of an unknown task
# (tests/test_classic_control.py) and stays one; the first three keep their bare names, in this order.
CLASSIC_TASKS = {task.name: task for task in (
    ClassicTask("CartPole", "CLASSIC_CARTPOLE", 4, 2, 4, 500),
    ClassicTask("Pendulum", "CLASSIC_PENDULUM", 2, 1, 3, 200),
    ClassicTask("MountainCar", "CLASSIC_MOUNTAINCAR", 2, 3, 2, 200),
    ClassicTask("Acrobot-v1", "CLASSIC_ACROBOT", 4, 3, 6, 500),
    ClassicTask("MountainCarContinuous-v0", "CLASSIC_MOUNTAINCARCONTINUOUS", 2, 1, 2, 999),
)}


def _task(task) -> ClassicTask:
    if isinstance(task, ClassicTask):
        return task
    if task not in CLASSIC_TASKS:
        raise ValueError(f"unknown classic-control task {task!r}; known: {', '.join(CLASSIC_TASKS)}")
    return CLASSIC_TASKS[task]


def _rows(tensor, name: str, dtype, rows: int | None, width: int | None, device) -> None:
    """A contiguous ``[rows, width]`` (``width`` None: ``[rows]``, or ``[rows, 1]``) tensor of ``dtype`` on ``device``."""
    ok = isinstance(tensor, torch.Tensor) and tensor.dtype == dtype and tensor.device == device and tensor.is_contiguous()
    if ok and width is None:
        ok = tensor.dim() in (1, 2) and tensor.numel() == tensor.shape[0] and (rows is None or tensor.shape[0] == rows)
    elif ok:
        ok = tensor.dim() == 2 and tensor.shape[1] == width and (rows is None or tensor.shape[0] == rows)
    if not ok:
        shape = f"[{'rows' if rows is None else rows}{'' if width is None else f', {width}'}]"
        raise ValueError(f"{name} must be a contiguous {dtype} {shape} tensor on {device}; got {_describe(tensor)}")


def _state(task: ClassicTask, state, steps, episode, name: str) -> int:
    if not isinstance(state, torch.Tensor):
        raise ValueError(f"{name}: 'state' must be a tensor; got {_describe(state)}")
    N = state.shape[0] if state.dim() == 2 else -1
    _rows(state, f"{name}: 'state'", torch.float32, None, task.state_dim, state.device)
    _rows(steps, f"{name}: 'steps'", torch.int32, N, None, state.device)
    if episode is not None:
        _rows(episode, f"{name}: 'episode'", torch.int64, N, None, state.device)
    return N


def classic_step(task, action: torch.Tensor, state: torch.Tensor, steps: torch.Tensor, max_steps: int, *, _host: bool = False):
    """One step of every env as ONE launch (``cusrl_classic_step``): ``state [N, S]`` and ``steps [N]`` advance in place; returns
    fresh ``(next_observation [N, O], reward [N, 1], terminated [N, 1] bool, truncated [N, 1] bool)``.  ``action [N, A]``: the
    torque, or logits / one-hot rows of which the first maximal column is taken.  CPU tensors: the host restatement."""
    task = _task(task)
    N = _state(task, state, steps, None, "classic_step")
    _rows(action, "classic_step: 'action'", torch.float32, N, task.action_dim, state.device)
    device = state.device
    next_observation = torch.empty(N, task.observation_dim, dtype=torch.float32, device=device)
    reward = torch.empty(N, 1, dtype=torch.float32, device=device)
    terminated = torch.empty(N, 1, dtype=torch.bool, device=device)
    truncated = torch.empty(N, 1, dtype=torch.bool, device=device)
    arguments = (task.kind, action.data_ptr(), state.data_ptr(), steps.data_ptr(), int(max_steps), next_observation.data_ptr(),
                 reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), N)
    if state.is_cuda:
        _checked.cusrl_classic_step(*arguments, _stream())
    else:
        if not _host:
            host_form("classic_step")
        check(_native.lib().cusrl_classic_step_cpu(*arguments), "cusrl_classic_step_cpu")
    _modified_in_place(state)
    _modified_in_place(steps)
    return next_observation, reward, terminated, truncated


def classic_reset(task, seed: int, indices: torch.Tensor, count: torch.Tensor | None, state: torch.Tensor, steps: torch.Tensor,
                  episode: torch.Tensor, max_steps: int, randomize_progress: bool = False, *, _host: bool = False) -> torch.Tensor:
    """``cusrl_classic_reset``, ONE launch: the envs ``indices[k]``, ``k < count``, start a new episode from Philox draws keyed
    on ``(seed, env, episode[env])`` (``state``, ``steps``, ``episode`` change in place, for those envs only); returns the fresh
    ``[len(indices), O]`` observation rows, row ``k`` belonging to env ``indices[k]`` — for ``k >= count`` its current
    observation.  ``count``: a 1-element int32 tensor beside ``state``, read by the launch and never by the host; None: every
    slot.  ``indices``: int64 ids in ``[0, N)``, distinct within the first ``count``.  CPU tensors: the host restatement."""
    task = _task(task)
    N = _state(task, state, steps, episode, "classic_reset")
    device = state.device
    _rows(indices, "classic_reset: 'indices'", torch.int64, None, None, device)
    if count is not None and not (isinstance(count, torch.Tensor) and count.dtype == torch.int32 and count.numel() == 1
                                  and count.device == device):
        raise ValueError(f"classic_reset: 'count' must be a 1-element int32 tensor on {device} or None; got {_describe(count)}")
    rows = indices.shape[0]
    observation = torch.empty(rows, task.observation_dim, dtype=torch.float32, device=device)
    arguments = (task.kind, int(seed) & 0xFFFFFFFFFFFFFFFF, indices.data_ptr(), _ptr(count), state.data_ptr(), steps.data_ptr(),
                 episode.data_ptr(), observation.data_ptr(), rows, int(bool(randomize_progress)), int(max_steps), N)
    if state.is_cuda:
        _checked.cusrl_classic_reset(*arguments, _stream())
    else:
        if not _host:
            host_form("classic_reset")
        check(_native.lib().cusrl_classic_reset_cpu(*arguments), "cusrl_classic_reset_cpu")
    for tensor in (state, steps, episode):
        _modified_in_place(tensor)
    return observation


def classic_step_cpu(task, action, state, steps, max_steps: int):
    """:func:`classic_step` by the library's host restatement, over CPU tensors (no ``host_form`` gate: asked for by name)."""
    if not (isinstance(state, torch.Tensor) and not state.is_cuda):
        raise ValueError(f"classic_step_cpu: 'state' must be a CPU tensor; got {_describe(state)}")
    return classic_step(task, action, state, steps, max_steps, _host=True)


def classic_reset_cpu(task, seed: int, indices, count, state, steps, episode, max_steps: int, randomize_progress: bool = False):
    """:func:`classic_reset` by the library's host restatement, over CPU tensors."""
    if not (isinstance(state, torch.Tensor) and not state.is_cuda):
        raise ValueError(f"classic_reset_cpu: 'state' must be a CPU tensor; got {_describe(state)}")
    return classic_reset(task, seed, indices, count, state, steps, episode, max_steps, randomize_progress, _host=True)


def _describe(value) -> str:
    if not isinstance(value, torch.Tensor):
        return type(value).__name__
    return f"{value.dtype} {tuple(value.shape)} on {value.device}{'' if value.is_contiguous() else ' (strided)'}"
