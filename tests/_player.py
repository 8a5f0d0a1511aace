"""Shared by tests/test_player.py (no GPU) and tests/test_player_gpu.py.  Imports no GPU.

Here: the scripted environment and agent of the golden (defined a second time in tests/golden/make_player_golden.py, which runs the
reference's ``Player`` over them), the numpy restatement of ``cusrl_play_epilogue`` the kernel is held to bit for bit, the done
patterns and guard-band helpers of the kernel tests, and the float64 recomputation of the play loop's outcome from saved arrays.

The lattice.  Kernel tests draw rewards as fp32 integers in {-2, ..., 2} (as tests/_mlp_backward.py does): every episode return,
ring entry and per-step reward sum is an integer far below 2^24, exact in fp32 and in the fp64 ``step_reward_sum`` in ANY order of
addition — the cross-block ``atomicAdd`` included — so every kernel assertion is ``torch.equal``."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"cusrl_play_epilogue", "cusrl_play_epilogue_workspace_words"}
N_ENVS, REWARD_DIM, TABLE_STEPS = 5, 2, 48
INVALID, UNSUPPORTED = -1, -3
GUARD = 64
PATTERNS = ("none", "all", "last", "block_heads", "bernoulli")


def block_size() -> int:
    """``kBlock`` as csrc/common.hpp declares it: the block edges of the kernel cases follow the source."""
    text = (ROOT / "cusrl_amd" / "csrc" / "common.hpp").read_text()
    return int(re.search(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", text).group(1))


def kernel_sizes() -> tuple[int, ...]:
    """{1, 255, 256, 257, 513, 4097} for a block of 256: one lane, a block's last lane, exactly one block, one lane into the second,
    one into the third, one into the seventeenth (the flag re-read of earlier blocks spans more than one 16-flag chunk per lane)."""
    b = block_size()
    return 1, b - 1, b, b + 1, 2 * b + 1, 16 * b + 1


# ------------------------------------------------------------------------------------------------ scripted env and agent
def make_tables(seed: int = 20251021):
    """``(reward [T, N, D] fp32, terminated [T, N] bool, truncated [T, N] bool)``; the environment walks them modulo T."""
    rs = np.random.RandomState(seed)
    reward = rs.standard_normal((TABLE_STEPS, N_ENVS, REWARD_DIM)).astype(np.float32)
    terminated = rs.random_sample((TABLE_STEPS, N_ENVS)) < 0.15
    truncated = rs.random_sample((TABLE_STEPS, N_ENVS)) < 0.10
    return reward, terminated, truncated


def scripted_classes(cusrl):
    """``(Environment, Agent)`` over the package ``cusrl`` (this one, or the reference in the generator).  The environment holds only
    arrays; observation = (step index, env index); the agent's action is ``observation[:, :1] * 0.5 + observation[:, 1:]``."""

    class ScriptedEnvironment(cusrl.Environment):
        def __init__(self, reward, terminated, truncated):
            steps, num, dim = reward.shape
            super().__init__(2, 1, num_instances=num, reward_dim=dim)
            self.reward, self.terminated, self.truncated = (torch.as_tensor(np.asarray(a)) for a in (reward, terminated, truncated))
            self.t = 0
            self.closed = 0

        def _observation(self, indices=None):
            ids = torch.arange(self.num_instances, dtype=torch.float32)
            observation = torch.stack((torch.full_like(ids, float(self.t)), ids), dim=-1)
            return observation if indices is None else observation[indices]

        def reset(self, *, indices=None, randomize_episode_progress=False):
            return self._observation(indices), None, {}

        def step(self, action):
            row = self.t % self.reward.shape[0]
            self.t += 1
            return (self._observation(), None, self.reward[row].clone(), self.terminated[row].unsqueeze(-1).clone(),
                    self.truncated[row].unsqueeze(-1).clone(), {})

        def close(self):
            self.closed += 1

    class ScriptedAgent(cusrl.Agent):
        def __init__(self, environment_spec):
            super().__init__(environment_spec, num_steps_per_update=1, device="cpu")

        def act(self, observation, state=None):
            observation = torch.as_tensor(observation).clone()
            self.transition = {"observation": observation, "action": observation[:, :1] * 0.5 + observation[:, 1:]}
            return self.transition["action"]

        def step(self, next_observation, reward, terminated, truncated, next_state=None, **kwargs):
            self.transition.update(reward=torch.as_tensor(reward), terminated=torch.as_tensor(terminated),
                                   truncated=torch.as_tensor(truncated))
            return super().step(next_observation, reward, terminated, truncated, next_state, **kwargs)

        def update(self):
            return {}

    return ScriptedEnvironment, ScriptedAgent


# ------------------------------------------------------------------------------------------------ restatement of the kernel
class EpilogueState:
    """Everything ``cusrl_play_epilogue`` carries from launch to launch, as numpy arrays in the kernel's dtypes."""

    def __init__(self, N: int, D: int, R: int):
        self.episode_rew = np.zeros((N, D), np.float32)
        self.episode_len = np.zeros(N, np.float32)
        self.ring_rew = np.zeros((R, D), np.float32)
        self.ring_len = np.zeros(R, np.float32)
        self.counter = np.zeros(2, np.int64)  # double-buffered: read at parity, written at parity ^ 1
        self.step_reward_sum = np.zeros(D, np.float64)
        self.episode_count = np.zeros(N, np.int64)


def play_epilogue_restated(state: EpilogueState, reward, terminated, truncated, parity: int, target: int):
    """One launch (include/cusrl_hip.h, ``cusrl_play_epilogue``): returns ``(done [N] bool, indices ascending, unfinished)``.
    Ring slots go to the finished envs in ASCENDING env order from ``counter[parity]`` on; the counter update is
    ``episode_count += done`` and the unfinished count is taken AFTER it (player.py:246,269)."""
    done = np.asarray(terminated).reshape(-1) | np.asarray(truncated).reshape(-1)
    indices = np.flatnonzero(done)
    R = state.ring_len.shape[0]
    assert indices.size <= R, "more finished envs than ring slots: the order of the overwrites is not defined"
    total = state.episode_rew + reward
    length = state.episode_len + np.float32(1)
    slots = (state.counter[parity] + np.arange(indices.size)) % R
    state.ring_rew[slots], state.ring_len[slots] = total[indices], length[indices]
    state.counter[parity ^ 1] = state.counter[parity] + indices.size
    state.episode_rew = np.where(done[:, None], np.float32(0), total)
    state.episode_len = np.where(done, np.float32(0), length)
    state.step_reward_sum = state.step_reward_sum + reward.astype(np.float64).sum(axis=0)
    state.episode_count = state.episode_count + done
    return done, indices, int((state.episode_count < target).sum())


def done_pattern(name: str, N: int, launch: int, seed: int = 7):
    """``(terminated, truncated)`` [N] bool of launch ``launch``; the two flags split the finished envs between them."""
    done = np.zeros(N, bool)
    if name == "all":
        done[:] = True
    elif name == "last":
        done[N - 1] = True
    elif name == "block_heads":
        done[:: block_size()] = True
    elif name == "bernoulli":
        done = np.random.RandomState(seed + 1000 * launch + N).random_sample(N) < 0.3
    elif name != "none":
        raise AssertionError(name)
    first = (np.arange(N) + launch) % 2 == 0
    both = np.arange(N) % 5 == 0
    return done & (first | both), done & (~first | both)


def lattice(shape, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(-2, 3, size=shape).astype(np.float32)


class Guarded:
    """A device tensor of exactly ``shape`` with ``GUARD`` poisoned elements on either side of it in the same allocation."""

    POISON = {torch.float32: 7777.0, torch.float64: 7777.0, torch.int64: 0x5A5A5A5A, torch.int32: 0x5A5A5A, torch.uint8: 1}

    def __init__(self, values, dtype, device):
        values = torch.as_tensor(np.ascontiguousarray(values))
        store = torch.uint8 if dtype is torch.bool else dtype
        self.whole = torch.full((values.numel() + 2 * GUARD,), self.POISON[store], dtype=store, device=device)
        middle = self.whole[GUARD : GUARD + values.numel()]
        middle.copy_(values.reshape(-1).to(store))
        self.tensor = (middle.view(torch.bool) if dtype is torch.bool else middle).view(values.shape)

    def intact(self) -> bool:
        poison = self.whole.new_tensor(self.POISON[self.whole.dtype])
        return bool((self.whole[:GUARD] == poison).all() and (self.whole[-GUARD:] == poison).all())


def check_error_codes(lib) -> None:
    """Host-side argument checks of ``cusrl_play_epilogue``: nothing is launched (the pointers are never dereferenced)."""
    p = 4096  # any non-NULL address
    limit = int(lib.cusrl_step_epilogue_max_envs())
    good = [p] * 12 + [8, 2, 8, 0, p, 1, p, p, None]  # ..., N, D, R, parity, episode_count, target, unfinished_out, workspace, stream

    def call(**changes):
        args = list(good)
        for position, value in changes.items():
            args[int(position[1:])] = value
        return lib.cusrl_play_epilogue(*args)

    assert call(_12=limit + 1, _14=limit + 1) == UNSUPPORTED
    assert call(_17=0) == INVALID and call(_17=-3) == INVALID
    for pointer in (16, 18, 19):  # episode_count, unfinished_out, workspace
        assert call(**{f"_{pointer}": None}) == INVALID
    for pointer in range(12):  # every pointer of the step epilogue
        assert call(**{f"_{pointer}": None}) == INVALID
    for size in (12, 13, 14):
        assert call(**{f"_{size}": 0}) == INVALID and call(**{f"_{size}": -1}) == INVALID
    assert call(_15=2) == INVALID
    assert int(lib.cusrl_play_epilogue_workspace_words()) == 2


# ------------------------------------------------------------------------------------------------ the loop, recomputed
def recompute_play(reward, done, target: int | None, ring: int):
    """From saved ``reward [T, N, D]`` and ``done [T, N]`` alone, in float64: the first step count at which every env has
    finished ``target`` episodes (None: T), the counters there, the three metrics of the reference's report (player.py:273-278 over
    trainer.py:54-94) and, per metric, the standard bound of recursive fp32 summation ``k * 2^-24 * sum |terms|`` with ``k`` the
    longest addition chain that metric goes through."""
    reward, done = np.asarray(reward, np.float64), np.asarray(done, bool)
    T, N, D = reward.shape
    counts = np.cumsum(done, axis=0)
    steps = T
    if target is not None:
        reached = np.flatnonzero((counts >= target).all(axis=1))
        assert reached.size, "the saved run never reaches the episode target"
        steps = int(reached[0]) + 1
    episode_rew, episode_abs, episode_len = np.zeros((N, D)), np.zeros((N, D)), np.zeros(N)
    ring_rew, ring_abs, ring_len, finished = np.zeros((ring, D)), np.zeros((ring, D)), np.zeros(ring), 0
    longest = 0
    for t in range(steps):
        episode_rew += reward[t]
        episode_abs += np.abs(reward[t])
        episode_len += 1
        for n in np.flatnonzero(done[t]):
            slot = finished % ring
            ring_rew[slot], ring_abs[slot], ring_len[slot] = episode_rew[n], episode_abs[n], episode_len[n]
            longest = max(longest, int(episode_len[n]))
            finished += 1
            episode_rew[n], episode_abs[n], episode_len[n] = 0.0, 0.0, 0.0
    filled = min(finished, ring)
    eps = 2.0 ** -24
    metrics = {
        "Mean step reward": reward[:steps].mean(axis=(0, 1)),
        "Mean episode reward": ring_rew[:filled].mean(axis=0) if filled else np.zeros(D),
        "Mean episode length": ring_len[:filled].mean() if filled else 0.0,
    }
    bounds = {
        # N rewards of a step are summed, then the steps: a chain of N + T additions
        "Mean step reward": (N + steps) * eps * np.abs(reward[:steps]).sum(axis=(0, 1)) / (steps * N),
        # an episode's return is a chain of its length, the ring's mean a chain of the ring size
        "Mean episode reward": (longest + ring) * eps * ring_abs[:filled].sum(axis=0) / max(filled, 1),
        "Mean episode length": (longest + ring) * eps * ring_len[:filled].sum() / max(filled, 1),
    }
    return steps, counts[steps - 1], metrics, bounds
