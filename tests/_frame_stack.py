"""Shared by tests/test_frame_stack.py and tests/test_frame_stack_gpu.py: the yardstick and the inputs.

The reference project has no frame stack, so nothing is recorded under tests/golden/.  The independent statement of the semantics
is :class:`DequeStack` below: gymnasium's documented ``FrameStackObservation(env, stack_size, padding_type)`` restated in numpy —
one ``deque(maxlen=stack_size)`` per env, filled at ``reset`` with ``stack_size - 1`` padding frames (the reset observation
itself for ``"reset"``, zeros for ``"zero"``) and the reset observation, appended to at ``step``, read oldest first.  It works on
the ``uint32`` view of the frames: the kernels move words, so every comparison is equality of bits."""

from __future__ import annotations

from collections import deque

import numpy as np
import torch

from cusrl_amd.template.environment import Environment

# a quiet NaN with a payload, a signalling NaN with a payload and the sign bit, -0.0, +Inf, -Inf, a denormal
SPECIAL_WORDS = (0x7FC12345, 0xFF812345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001)


class DequeStack:
    def __init__(self, num_envs: int, stack_size: int, padding_type: str = "reset", columns=None):
        assert padding_type in ("reset", "zero")
        self.stack_size, self.padding_type, self.columns = stack_size, padding_type, columns
        self.frames = [None] * num_envs

    def _frame(self, observation) -> np.ndarray:
        frame = np.ascontiguousarray(observation, dtype=np.float32).view(np.uint32)
        return frame.copy() if self.columns is None else frame[list(self.columns)].copy()

    def reset(self, env: int, observation) -> None:
        frame = self._frame(observation)
        padding = frame if self.padding_type == "reset" else np.zeros_like(frame)
        self.frames[env] = deque([padding.copy() for _ in range(self.stack_size - 1)], maxlen=self.stack_size)
        self.frames[env].append(frame)

    def step(self, env: int, observation) -> None:
        self.frames[env].append(self._frame(observation))

    def row(self, env: int) -> np.ndarray:
        return np.concatenate(list(self.frames[env]))

    def rows(self) -> np.ndarray:
        return np.stack([self.row(env) for env in range(len(self.frames))])


def words(tensor: torch.Tensor) -> torch.Tensor:
    """The int32 view of an fp32 tensor, on the host."""
    return tensor.detach().cpu().contiguous().view(torch.int32)


def expected(rows: np.ndarray) -> torch.Tensor:
    """uint32 rows of a :class:`DequeStack` as what :func:`words` returns."""
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int32))


def frames(seed: int, *shape: int) -> np.ndarray:
    """Seeded fp32 frames of ``shape`` with every word of :data:`SPECIAL_WORDS` in them (from 6 elements on; below that as many as
    fit), at positions spread over the array."""
    rng = np.random.RandomState(seed)
    data = (rng.standard_normal(shape) * 3).astype(np.float32)
    flat = data.reshape(-1).view(np.uint32)
    stride = flat.size // len(SPECIAL_WORDS)  # (distinct positions: i * stride + seed, mod the size, for i < 6 <= size / stride)
    for i, word in enumerate(SPECIAL_WORDS[: flat.size]):
        flat[(i * stride + seed) % flat.size if stride else i] = word
    return data


def offset_view(tensor: torch.Tensor) -> torch.Tensor:
    """The same values as a contiguous view one float behind a 16-byte boundary (what sends the kernels down their 4-byte
    path)."""
    flat = torch.empty(tensor.numel() + 1, dtype=tensor.dtype, device=tensor.device)
    view = flat[1:].view(tensor.shape)
    view.copy_(tensor)
    assert view.is_contiguous() and (view.numel() == 0 or view.data_ptr() % 16 == 4)
    return view


# The scripted sequence of the host tests: 3 envs, 6 steps; env 0 resets after step 0, env 1 after steps 2 and 3 (two consecutive
# steps), env 2 never.
SCRIPT_ENVS, SCRIPT_STEPS = 3, 6
SCRIPT_RESETS = {0: [0], 2: [1], 3: [1]}


class ScriptedEnvironment(Environment):
    """A host env that plays tables: observation ``table[t]`` at step ``t``, ``done`` by :data:`SCRIPT_RESETS`-like scripts
    (terminated on even steps, truncated on odd ones), reward ``t + env / 10``, a privileged state ``[N, 2]`` and an info entry; a
    reset returns ``reset_table[number of resets so far]`` rows.  No autoreset."""

    def __init__(self, table: np.ndarray, reset_table: np.ndarray, resets: dict, **properties):
        steps, num_envs, width = table.shape
        super().__init__(width, 2, num_instances=num_envs, state_dim=2, reward_dim=1, device="cpu", timestep=0.02, **properties)
        self.table, self.reset_table, self.resets = torch.from_numpy(table), torch.from_numpy(reset_table), resets
        self.t, self.reset_calls, self.closed = 0, 0, False

    def _state(self, rows):
        return torch.stack([torch.full((len(rows),), float(self.t)), torch.as_tensor(rows, dtype=torch.float32)], dim=1)

    def reset(self, *, indices=None, randomize_episode_progress: bool = False):
        rows = list(range(self.num_instances)) if indices is None else [int(i) for i in indices]
        observation = self.reset_table[self.reset_calls][rows].clone()
        self.reset_calls += 1
        return observation, self._state(rows), {"reset_call": self.reset_calls}

    def step(self, action):
        t = self.t
        done = torch.zeros(self.num_instances, 1, dtype=torch.bool)
        done[self.resets.get(t, [])] = True
        empty = torch.zeros_like(done)
        terminated, truncated = (done, empty) if t % 2 == 0 else (empty, done)
        reward = torch.full((self.num_instances, 1), float(t)) + torch.arange(self.num_instances).view(-1, 1) / 10
        self.t += 1
        return self.table[t].clone(), self._state(range(self.num_instances)), reward, terminated, truncated, {"step": t}

    def get_metrics(self):
        return {"scripted": 1.0}

    def state_dict(self):
        return {"t": self.t}

    def close(self):
        self.closed = True
