"""Inputs and an independent float64 restatement of ``RewardNormalization`` (cusrl_amd/hook/mdp/reward.py), shared by
tests/test_reward_normalization.py (host form) and tests/test_reward_normalization_gpu.py (kernel).

The restatement is written from the hook's description, not from the C body: the discounted return in fp32 with one rounding per
operation (that IS the specification), the batch mean and population variance from exactly rounded sums (``math.fsum``), the merge
in gymnasium's ``update_mean_var_count_from_moments`` form (moment sums, where the kernel uses weights), the scale and the division in
float64."""

import math
from types import SimpleNamespace

import numpy as np
import torch

GAMMA, EPSILON, STEPS = 0.99, 1e-8, 6
# 1025: one past 1024 rows; 4099: one chunk past the first stride of the kernel's 1024 threads x 4-row chunks, with a ragged chunk
SIZES = (1, 3, 257, 1025, 4099)
COLUMNS = (1, 2)
CASES = [(N, R) for N in SIZES for R in COLUMNS]

# Achieved error of the library's host restatement against the float64 restatement below, max |got - f64| / max(1, |f64|) over every
# case, step and element (measured; tests/test_reward_normalization.py prints the figures).  The host form asserts 2 x, the kernel 4 x.
HOST_ERROR = {"stats": 2.3e-15, "reward": 9.6e-8}


def inputs(N: int, R: int):
    """6 steps of seeded rewards of mixed sign and magnitude 1e-3 .. 1e2, and flags that finish some envs on every step (N >= 3)
    and env 0 on two steps in a row (2 and 3)."""
    rng = np.random.default_rng(1000 * N + R)
    reward = (rng.choice([-1.0, 1.0], size=(STEPS, N, R)) * 10.0 ** rng.uniform(-3.0, 2.0, size=(STEPS, N, R))).astype(np.float32)
    step, env = np.meshgrid(np.arange(STEPS), np.arange(N), indexing="ij")
    terminated = (env + step) % 5 == 0
    truncated = ((env + 2 * step) % 7 == 3) & ~terminated
    terminated[2:4, 0], truncated[2:4, 0] = True, False
    return reward, terminated, truncated


def restate(reward, terminated, truncated, gamma=GAMMA, epsilon=EPSILON, clip=None, update=True):
    """Per step: ``dict(returns [N, R] fp32, stats [3, R] float64, reward [N, R] float64)``."""
    steps, N, R = reward.shape
    G = np.zeros((N, R), np.float32)
    mean, var, count = [0.0] * R, [1.0] * R, [1e-4] * R
    out = []
    for t in range(steps):
        G = G * np.float32(gamma) + reward[t]
        assert G.dtype == np.float32
        if update:
            for c in range(R):
                column = [float(x) for x in G[:, c]]
                batch_mean = math.fsum(column) / N
                batch_var = math.fsum((x - batch_mean) ** 2 for x in column) / N
                total = count[c] + N
                delta = batch_mean - mean[c]
                m2 = var[c] * count[c] + batch_var * N + delta * delta * count[c] * N / total
                mean[c], var[c], count[c] = mean[c] + delta * N / total, m2 / total, total
        scaled = reward[t].astype(np.float64) / np.sqrt(np.asarray(var) + epsilon)
        if clip is not None:
            scaled = np.clip(scaled, -clip, clip)
        G = np.where((terminated[t] | truncated[t])[:, None], np.float32(0.0), G)
        out.append(dict(returns=G.copy(), stats=np.array([mean, var, count]), reward=scaled))
    return out


def run(op, device, reward, terminated, truncated, gamma=GAMMA, epsilon=EPSILON, clip=None, update=True):
    """The same steps through ``op`` (``ops.reward_normalize_`` or its ``_cpu_`` form) on ``device``: per step the CPU copies of
    ``dict(returns, stats, reward)``."""
    steps, N, R = reward.shape
    G = torch.zeros(N, R, device=device)
    stats = torch.tensor([[0.0] * R, [1.0] * R, [1e-4] * R], dtype=torch.float64, device=device)
    out = []
    for t in range(steps):
        r = torch.from_numpy(reward[t].copy()).to(device)  # (a copy: on the CPU `to` would alias the shared inputs)
        op(r, G, torch.from_numpy(terminated[t].copy()).to(device), torch.from_numpy(truncated[t].copy()).to(device), stats, gamma, epsilon,
           clip, update)
        out.append(dict(returns=G.cpu().clone(), stats=stats.cpu().clone(), reward=r.cpu()))
    return out


def error(got, expected) -> float:
    """max |got - f64| / max(1, |f64|)"""
    got, expected = np.asarray(got, np.float64), np.asarray(expected, np.float64)
    return float(np.max(np.abs(got - expected) / np.maximum(1.0, np.abs(expected)))) if got.size else 0.0


def errors(result, expected) -> dict:
    """The two figures of a run against the restatement, the returns asserted to the bit on the way."""
    figures = {"stats": 0.0, "reward": 0.0}
    for got, want in zip(result, expected):
        assert np.array_equal(got["returns"].numpy(), want["returns"])
        for key in figures:
            figures[key] = max(figures[key], error(got[key].numpy(), want[key]))
    return figures


def stub_agent(N: int, R: int, device="cpu"):
    """What ``RewardNormalization`` reads of its agent."""
    device = torch.device(device)
    return SimpleNamespace(parallelism=N, environment_spec=SimpleNamespace(reward_dim=R), inference_mode=False, device=device,
                           setup_module=lambda module: module.to(device))


def make_hook(cusrl, N: int, R: int, device="cpu", **kwargs):
    hook = cusrl.hook.RewardNormalization(**kwargs)
    hook.pre_init(stub_agent(N, R, device))
    hook.init()
    return hook
