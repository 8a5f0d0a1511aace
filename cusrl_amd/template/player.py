"""The play loop: drive a trained agent through an environment, call hooks, report (counterpart of cusrl/template/player.py:24-290).

Same constructor, attributes, hooks, SIGINT handling, metrics report and table as the reference, plus ``device_bookkeeping``:

* ``False`` — the reference's loop, statement for statement: ``get_done_indices`` (``nonzero`` + ``tolist``), a host ``episode_count``,
  ``stats.track_step`` / ``track_episode``.  Also what every env the kernel does not take gets (NumPy / CPU envs, other dtypes or
  shapes, more envs than ``cusrl_step_epilogue_max_envs()``: the conditions of ``Trainer._epilogue_applies_now``).
* ``True`` / ``None`` (``None``: decided by the first step's tensors) — ONE launch behind ``env.step`` does the bookkeeping of the
  step: ``cusrl_play_epilogue`` when ``num_episodes`` is set (done flag, episode statistics, ordered finished-env indices and their
  count, ``episode_count += done``, number of envs below the episode target), plain ``cusrl_step_epilogue`` otherwise.
  ``episode_count`` is then a device ``int64`` tensor.  A ``capturable`` env is reset through ``reset_static`` +
  ``ops.scatter_rows`` by the device-side count: with ``num_steps`` only a step reads nothing back, with ``num_episodes`` the host
  polls ONE pinned word (the unfinished count) after ``agent.step`` and the hooks have been issued.  Other envs — and any run with
  a hook that overrides ``PlayerHook.reset`` — wait for the finished count in pinned memory, as the trainer's fused path does; such
  a hook receives the finished indices as an ascending ``int64`` device tensor (``.tolist()`` gives the reference's list).

The play step is not captured in a graph; an agent built with ``compile=True`` replays its act step as it does in training."""

from __future__ import annotations

import signal
from collections.abc import Callable, Iterable
from typing import Any

import torch

from cusrl_amd import utils
from cusrl_amd.template.agent import Agent, AgentFactory
from cusrl_amd.template.environment import Environment, get_done_indices, update_observation_and_state
from cusrl_amd.template.trainer import EnvironmentStats, Trainer
from cusrl_amd.template.trial import Trial
from cusrl_amd.utils.nest import flatten_nested

__all__ = ["Player", "PlayerHook", "PlayerHookComposite"]


class PlayerHook:
    """Callbacks of the play loop; every one is a no-op until overridden (``:24-70``)."""

    player: "Player"
    agent: Agent
    environment: Environment

    def init(self, player: "Player"):
        self.player = player
        self.agent = player.agent
        self.environment = player.environment

    def step(self, step: int, transition: dict[str, Any]):
        """After every env step: the zero-based step index and the agent's transition."""

    def reset(self, indices):
        """When instances finished an episode: their indices — a list from the host bookkeeping, an ascending int64 device
        tensor from the device bookkeeping."""

    def close(self):
        """Once, when the loop ends (also when it raises)."""


class PlayerHookComposite(PlayerHook, list):
    """Delegates every callback to the contained hooks in registration order (``:73-91``)."""

    def init(self, player: "Player"):
        super().init(player)
        for hook in self:
            hook.init(player)

    def step(self, step: int, transition):
        for hook in self:
            hook.step(step, transition)

    def reset(self, indices):
        for hook in self:
            hook.reset(indices)

    def close(self):
        for hook in self:
            hook.close()

    def overrides_reset(self) -> bool:
        return any(getattr(type(hook), "reset", None) is not PlayerHook.reset for hook in self)


class _NoProgressBar:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def update(self):
        pass


def _progress_bar(total: int | None, enabled: bool):
    """tqdm's bar when asked for and installed (tqdm is optional here); else no bar."""
    if enabled:
        try:
            from tqdm import tqdm
        except ImportError:
            return _NoProgressBar()
        return tqdm(total=total, dynamic_ncols=True)
    return _NoProgressBar()


class Player:
    Hook = PlayerHook

    def __init__(self, environment: Environment | Callable[[], Environment], agent: Agent | AgentFactory,
                 checkpoint_path: str | Trial | None = None, num_steps: int | None = None, num_episodes: int | None = None,
                 timestep: float | None = None, deterministic: bool = True, verbose: bool = True,
                 progress_bar: bool | None = None, hooks: Iterable[PlayerHook] = (), device_bookkeeping: bool | None = None):
        self.environment = environment if isinstance(environment, Environment) else environment()
        self.agent = agent if isinstance(agent, Agent) else agent.from_environment(self.environment)
        self.trial: Trial | None = None
        if checkpoint_path is not None:
            self.trial = Trial(checkpoint_path) if isinstance(checkpoint_path, str) else checkpoint_path
            checkpoint = self.trial.load_checkpoint(map_location=self.agent.device)
            self.agent.load_state_dict(checkpoint["agent"])
            self.environment.load_state_dict(checkpoint["environment"])
        self.agent.set_inference_mode(deterministic=deterministic)
        self.num_steps = num_steps
        self.num_episodes = num_episodes
        self.timestep = self.environment.spec.timestep if timestep is None else timestep
        self.deterministic = deterministic
        self.verbose = verbose
        if progress_bar is None:
            progress_bar = num_steps is not None or num_episodes is not None
        self.progress_bar = progress_bar

        self.step_count = 0
        if num_episodes is not None and num_episodes < 1 and device_bookkeeping is not False:
            device_bookkeeping = False  # (a target below 1 ends the reference's loop after one step; the kernel takes none)
        self.device_bookkeeping = device_bookkeeping  # None until the first step has decided
        self.stats = self._make_stats(on_device=device_bookkeeping is not False)
        self.episode_count = torch.zeros(self.environment.num_instances, dtype=torch.long)
        self.interrupted = False
        self._scratch: dict[str, Any] = {}

        self.hook = PlayerHookComposite()
        for hook in hooks:
            self.register_hook(hook)

    def _make_stats(self, on_device: bool) -> EnvironmentStats:
        env = self.environment
        return EnvironmentStats(env.num_instances, env.spec.reward_dim, buffer_size=env.num_instances, device=env.spec.device,
                                on_device=on_device)

    def register_hook(self, hook: PlayerHook) -> "Player":
        hook.init(self)
        self.hook.append(hook)
        return self

    # ------------------------------------------------------------------ the loop
    def run_playing_loop(self) -> dict[str, float]:
        """Reset, then act / step / hooks / resets until ``num_steps`` env steps have run, every instance has finished
        ``num_episodes`` episodes, or SIGINT arrives (``:204-256``).  Returns the metrics it prints."""
        observation, state, _ = self.environment.reset()
        rate = utils.Rate(1 / self.timestep) if self.timestep is not None and self.timestep > 0 else None
        try:
            prev_handler = signal.signal(signal.SIGINT, self._sigint_handler)
        except ValueError:  # not the main thread
            prev_handler = None
        try:
            with _progress_bar(self.num_steps, self.progress_bar) as progress_bar:
                while (self.num_steps is None or self.step_count < self.num_steps) and not self.interrupted:
                    action = self.agent.act(observation, state)
                    observation, state, reward, terminated, truncated, info = self.environment.step(action)
                    if self._on_device(reward, terminated, truncated, info):
                        observation, state, finished = self._device_step(observation, state, reward, terminated, truncated, info)
                    else:
                        observation, state, finished = self._host_step(observation, state, reward, terminated, truncated, info)
                    if rate is not None:
                        rate.tick()
                    progress_bar.update()
                    if finished:
                        break
        finally:
            self.hook.close()
            self.environment.close()
            if prev_handler is not None:
                signal.signal(signal.SIGINT, prev_handler)
        metrics = self._get_metrics_report()
        self._display_metrics(metrics)
        return metrics

    def _host_step(self, observation, state, reward, terminated, truncated, info):
        """The reference's step (``:231-247``)."""
        self.agent.step(observation, reward, terminated, truncated, state, **info)
        self._step_event(observation, state, reward, terminated, truncated, info)
        if done_indices := get_done_indices(terminated, truncated):
            if not self.environment.spec.autoreset:
                init_observation, init_state, _ = self.environment.reset(indices=done_indices)
                observation, state = update_observation_and_state(observation, state, done_indices, init_observation, init_state)
            self._reset_event(done_indices)
        finished = self.num_episodes is not None and bool((self.episode_count >= self.num_episodes).all())
        return observation, state, finished

    def _on_device(self, reward, terminated, truncated, info) -> bool:
        """Does this step go through the one-launch epilogue?  Decided by the first step, then held."""
        if self.device_bookkeeping is False:
            return False
        applies = self.stats.on_device and Trainer._epilogue_applies_now(self, reward, terminated, truncated, info)
        if self.step_count == 0 and not applies:
            # nothing has been tracked yet: the reference's form takes over (over device tensors when the env has them)
            self.device_bookkeeping = False
            if self.stats.on_device:
                self.stats = self._make_stats(on_device=False)
            return False
        if not applies:
            raise RuntimeError("Player: the environment's step outputs stopped being what the fused step epilogue takes (device fp32 "
                               "[N, D] reward, [N, 1] bool flags); run with device_bookkeeping=False")
        self.device_bookkeeping = True
        if self.episode_count.device != self.stats.device:
            self.episode_count = self.episode_count.to(self.stats.device)
        return True

    def _device_step(self, observation, state, reward, terminated, truncated, info):
        from cusrl_amd import ops

        env, stats, scratch = self.environment, self.stats, self._scratch
        N, device = terminated.numel(), terminated.device
        static = bool(getattr(env, "capturable", False)) and not env.spec.autoreset
        hooked = self.hook.overrides_reset()
        if scratch.get("device") != device:
            scratch.update(device=device, indices=torch.zeros(N, dtype=torch.int64, device=device),
                           count=torch.zeros(1, dtype=torch.int32, device=device), done_counter=ops.HostCounter(),
                           unfinished=ops.HostCounter(), workspace=ops.play_epilogue_workspace(device))
        indices = scratch["indices"]
        # the finished count stays on the device unless the host needs it: to reset a non-capturable env, or for a reset hook
        host_count = hooked or (not static and not env.spec.autoreset)
        count = scratch["done_counter"].arm() if host_count else scratch["count"]
        done = torch.empty_like(terminated)
        if self.num_episodes is not None:
            stats.track_play(reward, terminated, truncated, done, indices, count, self.episode_count, self.num_episodes,
                             scratch["unfinished"].arm(), scratch["workspace"])
        else:
            stats.track_fused(reward, terminated, truncated, done, indices, count)
        self.agent.step(observation, reward, terminated, truncated, state, **{**info, "done": done})
        self.hook.step(self.step_count, self.agent.transition)
        self.step_count += 1

        if static:
            init_observation, init_state, _ = env.reset_static(indices, count)
            Trainer._splice_static(observation, state, indices, count, init_observation, init_state)
        if host_count:
            done_indices = indices[: scratch["done_counter"].wait()]
            if done_indices.numel():
                if not static and not env.spec.autoreset:
                    init_observation, init_state, _ = env.reset(indices=done_indices)
                    observation, state = Trainer._splice_resets(observation, state, done_indices, init_observation, init_state)
                if hooked:
                    self.hook.reset(done_indices.clone())  # (the index buffer is rewritten by the next step)
        finished = self.num_episodes is not None and scratch["unfinished"].wait() == 0
        return observation, state, finished

    def _sigint_handler(self, signum, frame):
        self.interrupted = True
        signal.signal(signal.SIGINT, signal.SIG_DFL)  # a second Ctrl+C kills at once

    def _step_event(self, observation, state, reward, terminated, truncated, info):
        self.stats.track_step(reward)
        self.hook.step(self.step_count, self.agent.transition)
        self.step_count += 1

    def _reset_event(self, done_indices: list[int]):
        self.episode_count[done_indices] += 1
        self.stats.track_episode(done_indices)
        self.hook.reset(done_indices)

    # ------------------------------------------------------------------ report
    def _get_metrics_report(self) -> dict[str, float]:
        if self.stats.on_device:
            episode_length, episode_reward, step_reward = self.stats.means()  # one host copy
        else:
            stats = self.stats
            step_reward, episode_reward, episode_length = stats.mean_step_reward, stats.mean_episode_reward, stats.mean_episode_length
        return {"Mean step reward": step_reward, "Mean episode reward": episode_reward,
                "Mean episode length": episode_length} | self.environment.get_metrics()

    def _display_metrics(self, metrics: dict[str, float]):
        if not metrics:
            return
        formatted = {key: f"{value: .6g}" for key, value in flatten_nested(metrics).items()}
        key_width = max(len(key) for key in formatted)
        value_width = max(len(value) for value in formatted.values())
        print("┌" + "─" * (key_width + 2) + "┬" + "─" * (value_width + 2) + "┐")
        for key, value in formatted.items():
            print(f"│ {key.ljust(key_width)} │ {value.ljust(value_width)} │")
        print("└" + "─" * (key_width + 2) + "┴" + "─" * (value_width + 2) + "┘")
