"""Rollout side: action sampling, the per-step epilogue and the synthetic benchmark env (``csrc/rollout.hip``)."""

from __future__ import annotations

import torch

from cusrl_amd.ops._common import _checked, _f32, _flag, _observed, _ptr, _stream, require_device


def normal_sample_logp(mean: torch.Tensor, std: torch.Tensor, eps: torch.Tensor, repeat_std: bool = False,
                       mean_bias: torch.Tensor | None = None):
    """``action = mean + eps * std`` and ``log_prob(action).sum(-1, keepdim=True)`` in one launch
    (cusrl/nn/module/distribution.py:198-205).  ``std`` may be the ``[A]`` vector a state-independent std repeats for every
    row; with ``repeat_std`` the launch also writes that repeated ``[B, A]`` matrix (what ``param.repeat(B, 1)`` gives,
    distribution.py:241-243) and returns it as a third value.  ``mean_bias`` ([A]): ``mean`` is the head's product without
    its bias; the launch adds it and returns the finished mean as the last value."""
    mean, std, eps = _f32(mean, "mean"), _f32(std, "std"), _f32(eps, "eps")
    A = mean.shape[-1]
    B = mean.numel() // A
    vector = std.dim() == 1 and std.numel() == A
    if (not vector and std.shape != mean.shape) or eps.shape != mean.shape:
        raise ValueError("normal_sample_logp: shape mismatch")
    action = torch.empty_like(mean)
    logp = torch.empty(mean.shape[:-1] + (1,), dtype=torch.float32, device=mean.device)
    repeated = torch.empty_like(mean) if (repeat_std and vector) else None
    finished = None
    if mean_bias is not None:
        mean_bias = _f32(mean_bias, "mean_bias")
        if mean_bias.numel() != A:
            raise ValueError("normal_sample_logp: one bias per action dim is required")
        finished = torch.empty_like(mean)
    _observed(
        "cusrl_normal_sample_logp", mean.data_ptr(), std.data_ptr(), eps.data_ptr(), action.data_ptr(), logp.data_ptr(),
        B, A, 1 if vector else B, _ptr(repeated), _ptr(mean_bias), _ptr(finished),
        nbytes=lambda: B * ((12 if vector else 16) * A + 4 + (4 * A if repeated is not None else 0) + (4 * A if finished is not None else 0)),
    )
    result = (action, logp)
    if repeat_std:
        result += (repeated if repeated is not None else std,)
    if finished is not None:
        result += (finished,)
    return result


def categorical_sample_logp(logits: torch.Tensor, noise: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """One-hot sample of ``softmax(logits)`` and its log-prob in one launch (cusrl/nn/module/distribution.py:332-366):
    ``argmax(softmax(logits) / noise)`` with ``noise ~ Exp(1)`` — torch.multinomial's own single-draw rule."""
    logits, noise = _f32(logits, "logits"), _f32(noise, "noise")
    if noise.shape != logits.shape:
        raise ValueError("categorical_sample_logp: shape mismatch")
    A = logits.shape[-1]
    B = logits.numel() // A
    action = torch.empty_like(logits)
    logp = torch.empty(logits.shape[:-1] + (1,), dtype=torch.float32, device=logits.device)
    _observed("cusrl_categorical_sample_logp", logits.data_ptr(), noise.data_ptr(), action.data_ptr(), logp.data_ptr(), B, A,
            nbytes=lambda: B * (12 * A + 4))
    return action, logp


def episode_stats(reward, done, episode_rew, episode_len, ring_rew, ring_len, num_episodes, step_reward_sum, parity: int) -> None:
    """One-launch ``EnvironmentStats.track_step`` + ``track_episode`` (cusrl/template/trainer.py:54-76), no host sync.
    ``num_episodes`` is the double-buffered int64[2] counter: read at ``parity``, written at ``parity ^ 1``."""
    if num_episodes.numel() != 2 or num_episodes.dtype != torch.int64:
        raise TypeError("episode_stats: 'num_episodes' must be the int64[2] double-buffered counter")
    reward = _f32(reward, "reward")
    done = _flag(done, "done")
    N, D = reward.shape
    _observed(
        "cusrl_episode_stats",
        reward.data_ptr(), done.data_ptr(), episode_rew.data_ptr(), episode_len.data_ptr(), ring_rew.data_ptr(),
        ring_len.data_ptr(), num_episodes.data_ptr(), step_reward_sum.data_ptr(), N, D, ring_len.numel(), int(parity),
        nbytes=lambda: N * (12 * D + 9),
    )


def step_epilogue(reward, terminated, truncated, done_out, episode_rew, episode_len, ring_rew, ring_len, num_episodes,
                  step_reward_sum, indices_out, count_out, parity: int) -> None:
    """``done = terminated | truncated`` + episode statistics + ordered finished-env indices and their count in ONE launch
    (``cusrl_step_epilogue``); ``count_out`` may be pinned host memory (:class:`HostCounter`)."""
    reward = _f32(reward, "reward")
    terminated, truncated = _flag(terminated, "terminated"), _flag(truncated, "truncated")
    N, D = reward.shape
    if terminated.numel() != N or truncated.numel() != N or done_out.numel() != N or indices_out.numel() < N:
        raise ValueError("step_epilogue: inconsistent sizes")
    if episode_rew.shape != (N, D) or episode_len.numel() != N or ring_rew.shape[-1] != D or step_reward_sum.numel() != D:
        raise ValueError(f"step_epilogue: the reward is [{N}, {D}] but the accumulators were built for "
                         f"{tuple(episode_rew.shape)} (an env returning another channel count than its spec says?)")
    _observed(
        "cusrl_step_epilogue",
        reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), done_out.data_ptr(), episode_rew.data_ptr(),
        episode_len.data_ptr(), ring_rew.data_ptr(), ring_len.data_ptr(), num_episodes.data_ptr(), step_reward_sum.data_ptr(),
        indices_out.data_ptr(), count_out.data_ptr(), N, D, ring_len.numel(), int(parity),
        nbytes=lambda: N * (12 * D + 11),
    )


def play_epilogue_workspace(device) -> torch.Tensor:
    """The zeroed ticket workspace of :func:`play_epilogue` — allocated (and zeroed) once, every launch leaves it zero."""
    from cusrl_amd import _native

    return torch.zeros(int(_native.lib().cusrl_play_epilogue_workspace_words()), dtype=torch.int32, device=device)


def play_epilogue(reward, terminated, truncated, done_out, episode_rew, episode_len, ring_rew, ring_len, num_episodes,
                  step_reward_sum, indices_out, count_out, parity: int, episode_count, target_episodes: int, unfinished_out,
                  workspace) -> None:
    """:func:`step_epilogue` of the play loop (``cusrl_play_epilogue``, ONE launch): on top of it ``episode_count += done``
    (int64 ``[N]``, in place) and ``unfinished_out`` = number of envs still below ``target_episodes`` (one int32 on the device or
    in pinned host memory).  ``workspace``: :func:`play_epilogue_workspace`, zero before and after every launch."""
    reward = _f32(reward, "reward")
    terminated, truncated = _flag(terminated, "terminated"), _flag(truncated, "truncated")
    require_device(episode_count, "episode_count"), require_device(workspace, "workspace")
    N, D = reward.shape
    if terminated.numel() != N or truncated.numel() != N or done_out.numel() != N or indices_out.numel() < N:
        raise ValueError("play_epilogue: inconsistent sizes")
    if episode_rew.shape != (N, D) or episode_len.numel() != N or ring_rew.shape[-1] != D or step_reward_sum.numel() != D:
        raise ValueError(f"play_epilogue: the reward is [{N}, {D}] but the accumulators were built for {tuple(episode_rew.shape)}")
    if episode_count.dtype != torch.int64 or episode_count.numel() != N or not episode_count.is_contiguous():
        raise TypeError("play_epilogue: 'episode_count' must be a contiguous int64 [N] device tensor")
    if unfinished_out.dtype != torch.int32 or unfinished_out.numel() != 1 or not (unfinished_out.is_cuda or unfinished_out.is_pinned()):
        raise TypeError("play_epilogue: 'unfinished_out' must be a 1-element int32 tensor on the device or in pinned host memory")
    if workspace.dtype != torch.int32 or workspace.numel() < 2 or not workspace.is_contiguous():
        raise TypeError("play_epilogue: 'workspace' must come from play_epilogue_workspace()")
    _observed(
        "cusrl_play_epilogue",
        reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), done_out.data_ptr(), episode_rew.data_ptr(),
        episode_len.data_ptr(), ring_rew.data_ptr(), ring_len.data_ptr(), num_episodes.data_ptr(), step_reward_sum.data_ptr(),
        indices_out.data_ptr(), count_out.data_ptr(), N, D, ring_len.numel(), int(parity), episode_count.data_ptr(),
        int(target_episodes), unfinished_out.data_ptr(), workspace.data_ptr(),
        nbytes=lambda: N * (12 * D + 11 + 16),
    )


class PendingStepEpilogue:
    """A step epilogue whose launch has been handed to the buffer push of the same env step (``cusrl_step_epilogue_push``:
    ONE launch for both).  ``launch()`` issues it on its own — the push could not take it."""

    __slots__ = ("args", "done_out")

    def __init__(self, reward, terminated, truncated, done_out, episode_rew, episode_len, ring_rew, ring_len, num_episodes,
                 step_reward_sum, indices_out, count_out, parity: int):
        self.args = (reward, terminated, truncated, done_out, episode_rew, episode_len, ring_rew, ring_len, num_episodes,
                     step_reward_sum, indices_out, count_out, parity)
        self.done_out = done_out

    def launch(self) -> None:
        step_epilogue(*self.args)

    def launch_with_push(self, table, count: int, done_field: int, cursor: int, parallelism: int) -> None:
        (reward, terminated, truncated, done_out, episode_rew, episode_len, ring_rew, ring_len, num_episodes, step_reward_sum,
         indices_out, count_out, parity) = self.args
        reward = _f32(reward, "reward")
        terminated, truncated = _flag(terminated, "terminated"), _flag(truncated, "truncated")
        N, D = reward.shape
        if terminated.numel() != N or truncated.numel() != N or done_out.numel() != N or indices_out.numel() < N or parallelism != N:
            raise ValueError("step_epilogue_push: inconsistent sizes")
        _observed(
            "cusrl_step_epilogue_push",
            reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), done_out.data_ptr(), episode_rew.data_ptr(),
            episode_len.data_ptr(), ring_rew.data_ptr(), ring_len.data_ptr(), num_episodes.data_ptr(), step_reward_sum.data_ptr(),
            indices_out.data_ptr(), count_out.data_ptr(), N, D, ring_len.numel(), int(parity), table, count, done_field, cursor,
            nbytes=lambda: N * (12 * D + 11) + sum(2 * parallelism * table[i].row_bytes for i in range(count)),
        )


def synthetic_env_step(seed: int, counter: torch.Tensor, num_envs: int, obs_dim: int, reward_dim: int, p_terminate: float,
                       p_truncate: float):
    """One step of the i.i.d. benchmark env as ONE launch (``cusrl_synthetic_env_step``): returns
    ``(next_observation [N, obs], reward [N, R], terminated [N, 1] bool, truncated [N, 1] bool, reset_rows [N, obs])``.
    ``counter``: int64[2] device tensor (zeros at construction) that the launch itself advances."""
    require_device(counter, "counter")
    dev = counter.device
    next_observation = torch.empty((num_envs, obs_dim), dtype=torch.float32, device=dev)
    reset_rows = torch.empty((num_envs, obs_dim), dtype=torch.float32, device=dev)
    reward = torch.empty((num_envs, reward_dim), dtype=torch.float32, device=dev)
    terminated = torch.empty((num_envs, 1), dtype=torch.bool, device=dev)
    truncated = torch.empty((num_envs, 1), dtype=torch.bool, device=dev)
    _checked.cusrl_synthetic_env_step(seed & 0xFFFFFFFFFFFFFFFF, counter.data_ptr(), num_envs, obs_dim, reward_dim,
            float(p_terminate), float(p_truncate), next_observation.data_ptr(), reward.data_ptr(), terminated.data_ptr(),
            truncated.data_ptr(), reset_rows.data_ptr(), _stream())
    return next_observation, reward, terminated, truncated, reset_rows
