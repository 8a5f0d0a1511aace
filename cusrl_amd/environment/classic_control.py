"""CartPole, Pendulum, MountainCar, Acrobot and MountainCarContinuous as device-resident environments (``csrc/environment.hip``; formulas and constants:
include/cusrl_hip.h; DESIGN.md §7, "Classic-control environments").

The reference takes these tasks from gymnasium (cusrl/environment/gym.py, zoo/gym/classic_control.py): a host simulator and a
host round trip per step.  Here the per-env state (``state [N, S]`` fp32, ``steps [N]`` int32, ``episode [N]`` int64) lives in
HBM, ``step`` is ONE launch and ``reset`` / ``reset_static`` are ONE launch; nothing is read by the host and nothing is drawn
from torch's generator, so the trainer replays whole env steps from hipGraphs (``capturable``, ``generator_free``).  On CPU
tensors the same calls run the library's host restatement of the kernels (behind ``utils.misc.host_form``)."""

from __future__ import annotations

import torch

from cusrl_amd.ops.environment import CLASSIC_TASKS, ClassicTask
from cusrl_amd.template.environment import Environment
from cusrl_amd.utils.config import device as resolve_device

__all__ = ["Acrobot", "CartPole", "ClassicControlEnvironment", "MountainCar", "MountainCarContinuous", "Pendulum", "make"]


class ClassicControlEnvironment(Environment):
    """Common part of the tasks; a subclass names its :class:`ClassicTask`.

    An env that finishes keeps its terminal state until it is reset (``autoreset = False``): the trainer resets it in the same
    env step, by ``reset_static`` (device-side count) or ``reset(indices=...)``.  Episode ``n`` of env ``e`` always starts from
    the same state for the same seed, whatever the number of envs, the order of the resets and the path they took."""

    task: ClassicTask

    def __init__(self, num_instances: int = 1, *, device=None, seed: int | None = None, max_episode_steps: int | None = None):
        device = resolve_device(device)
        task = self.task
        super().__init__(task.observation_dim, task.action_dim, num_instances=num_instances, reward_dim=1, device=device,
                         autoreset=False)
        self.device = device
        self.max_episode_steps = task.max_episode_steps if max_episode_steps is None else int(max_episode_steps)
        if self.max_episode_steps < 1:
            raise ValueError(f"max_episode_steps must be at least 1; got {max_episode_steps}")
        self.capturable = self.generator_free = self.device.type == "cuda"
        # follows set_global_seed (seed + rank) without consuming any generator, as SyntheticEnvironment's fused stream does
        base = torch.initial_seed() if seed is None else int(seed)
        self._seed = (base * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
        # (allocated once and only ever written in place: captured steps hold their addresses)
        self.state = torch.zeros(num_instances, task.state_dim, dtype=torch.float32, device=device)
        self.steps = torch.zeros(num_instances, dtype=torch.int32, device=device)
        self.episode = torch.zeros(num_instances, dtype=torch.int64, device=device)
        self._all = torch.arange(num_instances, dtype=torch.int64, device=device)

    def reset(self, *, indices=None, randomize_episode_progress: bool = False):
        from cusrl_amd import ops

        if indices is None:
            indices = self._all
        else:
            indices = torch.as_tensor(indices, dtype=torch.int64, device=self.device).reshape(-1).contiguous()
        observation = ops.classic_reset(self.task, self._seed, indices, None, self.state, self.steps, self.episode,
                                        self.max_episode_steps, randomize_episode_progress)
        return observation, None, {}

    def reset_static(self, indices, count):
        from cusrl_amd import ops

        observation = ops.classic_reset(self.task, self._seed, indices, count, self.state, self.steps, self.episode,
                                        self.max_episode_steps, False)
        return observation, None, {}

    def step(self, action):
        from cusrl_amd import ops

        next_observation, reward, terminated, truncated = ops.classic_step(self.task, action, self.state, self.steps,
                                                                           self.max_episode_steps)
        return next_observation, None, reward, terminated, truncated, {}

    def state_dict(self):
        return {"task": self.task.name, "seed": self._seed, "state": self.state.clone(), "steps": self.steps.clone(),
                "episode": self.episode.clone()}

    def load_state_dict(self, state_dict):
        if not state_dict:
            return
        if state_dict["task"] != self.task.name:
            raise ValueError(f"a {state_dict['task']} checkpoint cannot be loaded into {self.task.name}")
        if tuple(state_dict["state"].shape) != tuple(self.state.shape):
            raise ValueError(f"the checkpoint holds {state_dict['state'].shape[0]} envs, this environment {self.num_instances}")
        self._seed = int(state_dict["seed"])
        self.state.copy_(state_dict["state"])
        self.steps.copy_(state_dict["steps"])
        self.episode.copy_(state_dict["episode"])


class CartPole(ClassicControlEnvironment):
    """Balance a pole on a cart: observation ``(x, x', theta, theta')``, action logits over {left, right}, reward 1 per step,
    terminated beyond 2.4 m or 12 degrees, truncated at 500 steps."""

    task = CLASSIC_TASKS["CartPole"]


class Pendulum(ClassicControlEnvironment):
    """Swing a pendulum up: observation ``(cos theta, sin theta, theta')``, one torque in [-2, 2], reward
    ``-(theta^2 + 0.1 theta'^2 + 0.001 u^2)``, truncated at 200 steps."""

    task = CLASSIC_TASKS["Pendulum"]


class MountainCar(ClassicControlEnvironment):
    """Drive a weak car out of a valley: observation ``(position, velocity)``, action logits over {left, none, right}, reward -1
    per step, terminated at position 0.5, truncated at 200 steps."""

    task = CLASSIC_TASKS["MountainCar"]


class Acrobot(ClassicControlEnvironment):
    """Swing the tip of a two-link pendulum above the bar: observation ``(cos theta1, sin theta1, cos theta2, sin theta2, theta1',
    theta2')``, action logits over the torques {-1, 0, +1} on the second joint, one Runge-Kutta step of 0.2 s per env step, reward
    -1 per step (0 on the last), terminated when ``-cos theta1 - cos(theta1 + theta2) > 1``, truncated at 500 steps."""

    task = CLASSIC_TASKS["Acrobot-v1"]


class MountainCarContinuous(ClassicControlEnvironment):
    """MountainCar with one continuous force in [-1, 1]: observation ``(position, velocity)``, reward ``-0.1 a^2`` per step and
    +100 on reaching position 0.45, terminated there, truncated at 999 steps."""

    task = CLASSIC_TASKS["MountainCarContinuous-v0"]


# The bare names of the first three (in this order: the error message lists them first), then the gym ids of all five.  Acrobot and
# MountainCarContinuous have NO bare name: "Acrobot" is the suite's standing example of an unknown environment and stays one.
_REGISTRY = {cls.__name__: cls for cls in (CartPole, Pendulum, MountainCar)}
_REGISTRY.update({"CartPole-v1": CartPole, "Pendulum-v1": Pendulum, "MountainCar-v0": MountainCar, "Acrobot-v1": Acrobot,
                  "MountainCarContinuous-v0": MountainCarContinuous})


def make(name: str, num_instances: int = 1, *, frame_stack: int | None = None, **kwargs) -> Environment:
    """``make("CartPole", 64, device="cuda:0")``; the names: CartPole, Pendulum, MountainCar, and the gym ids CartPole-v1,
    Pendulum-v1, MountainCar-v0, Acrobot-v1, MountainCarContinuous-v0.  ``frame_stack=S`` wraps the task in
    ``FrameStack(env, S)`` (None: the bare task)."""
    if name not in _REGISTRY:
        raise ValueError(f"unknown environment {name!r}; available: {', '.join(_REGISTRY)}")
    env = _REGISTRY[name](num_instances, **kwargs)
    if frame_stack is None:
        return env
    from cusrl_amd.environment.frame_stack import FrameStack

    return FrameStack(env, frame_stack)
