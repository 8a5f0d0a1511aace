"""What tests/test_classic_control_more.py (host form) and tests/test_classic_control_more_gpu.py (kernels) share for Acrobot and
MountainCarContinuous: the input tables, a float64 evaluation of the two tasks' TEXTBOOK formulas (``cos(x - pi/2)``, unfolded
constants, a looped wrap: written independently of the C body, which folds the constants and wraps in closed form), and the reset
cases.  The error measure and the generic pieces are tests/_classic_control.py's, whose dicts are only read here.

``HOST_ERROR`` is the largest error of the library's host restatement against the float64 evaluation on these inputs, measured on
the build machine (x86-64, glibc's sinf / cosf / sincosf) and written into DESIGN.md §7; the CPU test asserts it with a factor 2,
the GPU test with a factor 4 (the device's sinf / cosf are not glibc's): the project's established margins."""

from __future__ import annotations

import numpy as np
import torch

from _classic_control import SEED, assert_exact_parts, run_step, scaled_error, step_error  # noqa: F401  (re-exported)

ACROBOT, CONTINUOUS = "Acrobot-v1", "MountainCarContinuous-v0"
TASKS = {ACROBOT: dict(S=4, A=3, O=6, max_steps=500), CONTINUOUS: dict(S=2, A=1, O=2, max_steps=999)}
# measured with tests/test_classic_control_more.py::test_host_restatement_against_float64 (it prints each figure before it asserts)
HOST_ERROR = {ACROBOT: 6.0e-6, CONTINUOUS: 5.4e-8}  # measured 5.908e-6, 5.343e-8
RANDOM_ROWS = 257
RANGES = {ACROBOT: [(-0.1, 0.1)] * 4, CONTINUOUS: [(-0.6, -0.4), (0.0, 0.0)]}
PI = np.pi

_F = np.float32(-1.2)  # (the clamp's own fp32 value: the table needs a position that IS the saturated one)


def inputs(name: str):
    """``(state [M, S] fp32, action [M, A] fp32, steps [M] int32, max_steps)``: the fixed table, then 257 seeded random rows."""
    rng = np.random.RandomState({ACROBOT: 14, CONTINUOUS: 15}[name])
    M, max_steps = RANDOM_ROWS, TASKS[name]["max_steps"]
    if name == ACROBOT:
        table = [  # theta1, theta2, theta1', theta2', logits, steps
            (0.0, 0.0, 0.0, 0.0, (1, 0, 0), 0), (0.0, 0.0, 0.0, 0.0, (0, 1, 0), 0), (0.0, 0.0, 0.0, 0.0, (0, 0, 1), 0),  # hanging at rest
            (0.1, -0.2, 0.3, -0.4, (0, 0, 0), 3),  # ties: column 0
            (0.1, -0.2, 0.3, -0.4, (1, 2, 2), 3),  # column 1
            (0.1, -0.2, 0.3, -0.4, (5, 1, 5), 3),  # column 0
            (3.0, 0.5, 2.0, 0.0, (0, 1, 0), 5), (-3.0, -0.5, -2.0, 0.0, (0, 1, 0), 5),  # raw theta1 leaves [-pi, pi] on either side
            (0.5, 3.0, 0.0, 3.0, (0, 0, 1), 5), (-0.5, -3.0, 0.0, -3.0, (1, 0, 0), 5),  # raw theta2 does
            (3.1, -3.1, 6.0, -9.0, (0, 1, 0), 5), (-3.1, 3.1, -6.0, 9.0, (0, 1, 0), 5),  # both, in opposite directions
            (0.0, 0.5, 12.5, 5.0, (0, 1, 0), 7), (0.0, -0.5, -12.5, -5.0, (0, 1, 0), 7),  # |theta1'| driven past 4 pi
            (0.0, 0.0, 0.0, 28.2, (0, 0, 1), 7), (0.0, 0.0, 0.0, -28.2, (1, 0, 0), 7),  # |theta2'| driven past 9 pi
            (2.8, 0.0, 0.0, 0.0, (0, 1, 0), 9),  # the tip above the line: terminated
            (2.15, 0.0, 0.0, 0.0, (0, 1, 0), 9),  # just below it
            (2.8, 0.1, 0.5, 0.0, (0, 0, 1), 499),  # terminated at the step limit: not truncated
            (0.3, 0.2, 0.1, 0.0, (0, 1, 0), 499),  # survives at the step limit: truncated
            (0.3, 0.2, 0.1, 0.0, (0, 1, 0), 498),  # one short of it
        ]
        state = np.array([row[:4] for row in table], dtype=np.float32)
        action = np.array([row[4] for row in table], dtype=np.float32)
        steps = np.array([row[5] for row in table], dtype=np.int32)
        random_state = rng.uniform(-1, 1, (M, 4)) * np.array([PI, PI, 4 * PI, 9 * PI])
        random_action = rng.randint(0, 2, (M, 3))  # (ties included)
    else:
        table = [  # position, velocity, action, steps
            (_F, -0.01, -1.0, 0),  # at the left wall moving left: velocity zeroed
            (_F, 0.02, 1.0, 0), (-0.5, 0.07, 1.0, 4), (-0.5, -0.07, -1.0, 4),  # v = +-0.07 pushed further
            (0.6, 0.05, 1.0, 4),  # p = 0.6 pushed further; terminated
            (0.43, 0.03, 0.0, 4),  # crosses 0.45 with v >= 0
            (0.40, 0.03, 0.5, 4),  # stops short of it
            (-0.5, 0.0, 1.7, 6), (-0.5, 0.0, 1.0, 6),  # a > 1 gives the state of a = 1 and another reward
            (-0.5, 0.0, -2.5, 6), (-0.5, 0.0, -1.0, 6),  # a < -1 likewise
            (0.44, 0.05, 0.3, 998),  # terminated at the step limit: not truncated
            (-0.3, 0.01, 0.2, 998),  # survives at the step limit: truncated
            (-0.3, 0.01, 0.2, 997),  # one short of it
        ]
        state = np.array([row[:2] for row in table], dtype=np.float32)
        action = np.array([[row[2]] for row in table], dtype=np.float32)
        steps = np.array([row[3] for row in table], dtype=np.int32)
        random_state = rng.uniform(0, 1, (M, 2)) * np.array([1.8, 0.14]) + np.array([-1.2, -0.07])
        random_action = rng.uniform(-1.5, 1.5, (M, 1))
    random_steps = rng.randint(0, max_steps, M)
    random_steps[:4] = max_steps - 1
    state = np.concatenate([state, random_state.astype(np.float32)])
    action = np.concatenate([action, random_action.astype(np.float32)])
    steps = np.concatenate([steps, random_steps.astype(np.int32)])
    return torch.from_numpy(state), torch.from_numpy(action), torch.from_numpy(steps), max_steps


# ------------------------------------------------------------------------------------------------ Acrobot in float64
M1 = M2 = 1.0
L1 = 1.0
LC1 = LC2 = 0.5
I1 = I2 = 1.0
G = 9.8
DT = 0.2
MAX_VEL_1, MAX_VEL_2 = 4 * PI, 9 * PI


def acrobot_derivative(s: np.ndarray, a: np.ndarray) -> np.ndarray:
    """The textbook equations of motion, ``s [M, 4]`` (theta1, theta2, theta1', theta2') and the torque ``a [M]`` -> ``ds/dt``."""
    theta1, theta2, dtheta1, dtheta2 = s.T
    d1 = M1 * LC1**2 + M2 * (L1**2 + LC2**2 + 2 * L1 * LC2 * np.cos(theta2)) + I1 + I2
    d2 = M2 * (LC2**2 + L1 * LC2 * np.cos(theta2)) + I2
    phi2 = M2 * LC2 * G * np.cos(theta1 + theta2 - PI / 2)
    phi1 = (-M2 * L1 * LC2 * dtheta2**2 * np.sin(theta2) - 2 * M2 * L1 * LC2 * dtheta2 * dtheta1 * np.sin(theta2)
            + (M1 * LC1 + M2 * L1) * G * np.cos(theta1 - PI / 2) + phi2)
    ddtheta2 = (a + d2 / d1 * phi1 - M2 * L1 * LC2 * dtheta1**2 * np.sin(theta2) - phi2) / (M2 * LC2**2 + I2 - d2**2 / d1)
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.stack([dtheta1, dtheta2, ddtheta1, ddtheta2], axis=1)


def acrobot_rk4(s: np.ndarray, a: np.ndarray, dt: float) -> np.ndarray:
    """One classical Runge-Kutta step with the torque held; no wrap, no clamp."""
    k1 = acrobot_derivative(s, a)
    k2 = acrobot_derivative(s + dt / 2 * k1, a)
    k3 = acrobot_derivative(s + dt / 2 * k2, a)
    k4 = acrobot_derivative(s + dt * k3, a)
    return s + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def acrobot_energy(s: np.ndarray) -> np.ndarray:
    """Kinetic plus potential energy: what the continuous system conserves under zero torque."""
    theta1, theta2, dtheta1, dtheta2 = s.T
    d1 = M1 * LC1**2 + M2 * (L1**2 + LC2**2 + 2 * L1 * LC2 * np.cos(theta2)) + I1 + I2
    d2 = M2 * (LC2**2 + L1 * LC2 * np.cos(theta2)) + I2
    return (0.5 * d1 * dtheta1**2 + d2 * dtheta1 * dtheta2 + 0.5 * (M2 * LC2**2 + I2) * dtheta2**2
            - (M1 * LC1 + M2 * L1) * G * np.cos(theta1) - M2 * LC2 * G * np.cos(theta1 + theta2))


def _wrap(x: np.ndarray) -> np.ndarray:
    """The textbook wrap: ``while x > pi: x -= 2 pi; while x < -pi: x += 2 pi`` (finite inputs only)."""
    x = x.copy()
    assert np.isfinite(x).all()
    while (x > PI).any():
        x = np.where(x > PI, x - 2 * PI, x)
    while (x < -PI).any():
        x = np.where(x < -PI, x + 2 * PI, x)
    return x


def reference_step(name: str, state: torch.Tensor, action: torch.Tensor, steps: torch.Tensor, max_steps: int) -> dict:
    """The task's formulas in float64 from the fp32 inputs.  ``margin``: per row, how far the float64 result sits from the nearest
    threshold at which a flag or a discontinuous branch flips or a clamp starts to hold (Acrobot: the termination line, the raw
    angles against every odd multiple of pi, the raw velocities against 4 pi and 9 pi), in units of ``max(1, |threshold|)``.
    ``saturated``: the entries of the new state that are a clamp's bound (or the zeroed velocity) — constants, whatever the
    rounding before them.  (MountainCarContinuous's force clamp is continuous, flips nothing and leaves no constant in the state:
    it has no margin, so the table may hold a = +-1 itself.)"""
    s, a = state.numpy().astype(np.float64), action.numpy().astype(np.float64)
    rows = s.shape[0]
    saturated = np.zeros_like(s, dtype=bool)
    if name == ACROBOT:
        torque = np.argmax(a, axis=1) - 1.0
        raw = acrobot_rk4(s, torque, DT)
        theta1, theta2 = _wrap(raw[:, 0]), _wrap(raw[:, 1])
        saturated[:, 2], saturated[:, 3] = np.abs(raw[:, 2]) > MAX_VEL_1, np.abs(raw[:, 3]) > MAX_VEL_2
        new = np.stack([theta1, theta2, np.clip(raw[:, 2], -MAX_VEL_1, MAX_VEL_1), np.clip(raw[:, 3], -MAX_VEL_2, MAX_VEL_2)], axis=1)
        height = -np.cos(theta1) - np.cos(theta1 + theta2)
        terminated = height > 1.0
        reward = np.where(terminated, 0.0, -1.0)
        observation = np.stack([np.cos(theta1), np.sin(theta1), np.cos(theta2), np.sin(theta2), new[:, 2], new[:, 3]], axis=1)
        margin = np.abs(height - 1.0)
        for angle in (raw[:, 0], raw[:, 1]):  # the wrap's boundaries: +-pi, and +-3 pi where the number of turns changes
            for boundary in (PI, 3 * PI):
                margin = np.minimum(margin, np.abs(np.abs(angle) - boundary) / boundary)
        margin = np.minimum(margin, np.abs(np.abs(raw[:, 2]) - MAX_VEL_1) / MAX_VEL_1)
        margin = np.minimum(margin, np.abs(np.abs(raw[:, 3]) - MAX_VEL_2) / MAX_VEL_2)
    else:
        p, v = s.T
        force = np.clip(a[:, 0], -1.0, 1.0)
        raw_v = v + (force * 0.0015 - 0.0025 * np.cos(3 * p))
        new_v = np.clip(raw_v, -0.07, 0.07)
        raw_p = p + new_v
        new_p = np.clip(raw_p, -1.2, 0.6)
        wall = (new_p == -1.2) & (new_v < 0)
        saturated[:, 1] = (np.abs(raw_v) > 0.07) | wall
        saturated[:, 0] = (raw_p < -1.2) | (raw_p > 0.6)
        clamped_v = new_v
        new_v = np.where(wall, 0.0, new_v)
        new = np.stack([new_p, new_v], axis=1)
        terminated = (new_p >= 0.45) & (new_v >= 0)
        reward = np.where(terminated, 100.0, 0.0) - 0.1 * a[:, 0] ** 2  # the RAW action
        observation = new.copy()
        # flips: p across 0.45; v across 0 while p >= 0.45; the wall branch (raw p across -1.2 while moving left, or v across 0 at
        # the wall); the clamps' edges
        margin = np.abs(new_p - 0.45)
        margin = np.minimum(margin, np.where(new_p >= 0.45, np.abs(new_v), np.inf))
        margin = np.minimum(margin, np.where(clamped_v < 0, np.abs(raw_p + 1.2) / 1.2, np.inf))
        margin = np.minimum(margin, np.where(raw_p <= -1.2, np.abs(clamped_v), np.inf))
        margin = np.minimum(margin, np.minimum(np.abs(np.abs(raw_v) - 0.07), np.minimum(np.abs(raw_p + 1.2) / 1.2, np.abs(raw_p - 0.6))))
    new_steps = steps.numpy().astype(np.int64) + 1
    truncated = (new_steps >= max_steps) & ~terminated
    assert margin.shape == (rows,)
    return dict(state=new, observation=observation, reward=reward[:, None], terminated=terminated[:, None], truncated=truncated[:, None],
                steps=new_steps, margin=margin, saturated=saturated, raw=raw if name == ACROBOT else np.stack([raw_p, raw_v], axis=1))


# ------------------------------------------------------------------------------------------------------------------- reset
def fresh(name: str, N: int, device):
    """A marked, non-zero env state: rows that a reset must not touch are recognisable."""
    S = TASKS[name]["S"]
    state = (torch.arange(N * S, dtype=torch.float32).reshape(N, S) * 0.001 + 0.3).to(device)
    steps = (torch.arange(N, dtype=torch.int32) % 50 + 7).to(device)
    episode = (torch.arange(N, dtype=torch.int64) % 5 + 2).to(device)
    return state, steps, episode


def observation_of(name: str, state: torch.Tensor) -> np.ndarray:
    s = state.cpu().numpy().astype(np.float64)
    if name == ACROBOT:
        return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]], axis=1)
    return s


def assert_observation(name: str, observation: torch.Tensor, state_rows: torch.Tensor, bound: float, where):
    """An observation row is its state row: the bits for MountainCarContinuous and Acrobot's two velocity columns, within ``bound``
    of the float64 cos / sin of the fp32 angles for Acrobot's first four columns."""
    if name == ACROBOT:
        assert torch.equal(observation[:, 4:].cpu(), state_rows[:, 2:].cpu()), where
        assert scaled_error(observation, observation_of(name, state_rows)) <= bound, where
    else:
        assert torch.equal(observation.cpu(), state_rows.cpu()), where


def reset_cases(reset_fn, name: str, device, N: int) -> dict:
    """Every case of tests/_classic_control.py's ``reset_cases`` for the two later tasks, through ``reset_fn``
    (``ops.classic_reset`` / ``ops.classic_reset_cpu``) on ``device``; asserts the properties and returns the produced tensors (on
    the CPU) so that two devices can be compared."""
    max_steps = TASKS[name]["max_steps"]
    bound = 4 * HOST_ERROR[ACROBOT]
    out = {}
    ascending = torch.arange(N, dtype=torch.int64, device=device)
    subset = torch.tensor([N - 1, 0, N // 2] if N >= 3 else [0], dtype=torch.int64, device=device)
    for label, indices in (("ascending", ascending), ("subset", subset)):
        rows = indices.numel()
        for count in (0, 1, rows, None):
            state, steps, episode = fresh(name, N, device)
            before = [t.clone() for t in (state, steps, episode)]
            count_t = None if count is None else torch.tensor([count], dtype=torch.int32, device=device)
            observation = reset_fn(name, SEED, indices, count_t, state, steps, episode, max_steps)
            live = rows if count is None else count
            changed = torch.zeros(N, dtype=torch.bool)
            changed[indices[:live].cpu()] = True
            where = (name, label, count, N)
            for after, old in zip((state, steps, episode), before):  # only the first `count` envs change
                assert torch.equal(after.cpu()[~changed], old.cpu()[~changed]), where
            assert torch.equal(episode.cpu()[changed], before[2].cpu()[changed] + 1), where
            assert (steps.cpu()[changed] == 0).all(), where
            for column, (lo, hi) in enumerate(RANGES[name]):  # draws in the documented ranges
                drawn = state.cpu()[changed][:, column].double()
                assert ((drawn >= np.float32(lo)) & (drawn <= np.float32(hi))).all(), where
                if live > 1 and hi > lo:
                    assert drawn.unique().numel() > 1, where
            # row k is env indices[k]: the fresh observation below the count, the current one above it
            assert observation.shape == (rows, TASKS[name]["O"]), where
            assert_observation(name, observation, state[indices], bound, where)
            out[(label, count)] = tuple(t.cpu() for t in (observation, state, steps, episode))
    # the same (seed, env, episode) gives the same row whatever N and launch order: all at once == one env at a time, backwards
    state, steps, episode = fresh(name, N, device)
    reset_fn(name, SEED, ascending, None, state, steps, episode, max_steps)
    state1, steps1, episode1 = fresh(name, N, device)
    for e in reversed(range(N)) if N <= 8 else (N - 1, 1, 0, N // 2):
        reset_fn(name, SEED, torch.tensor([e], dtype=torch.int64, device=device), None, state1, steps1, episode1, max_steps)
        assert torch.equal(state1[e], state[e]) and episode1[e] == episode[e], (name, e)
    # ... and inside a larger population
    state2, steps2, episode2 = fresh(name, N + 5, device)
    reset_fn(name, SEED, torch.arange(N + 5, dtype=torch.int64, device=device), None, state2, steps2, episode2, max_steps)
    same_episode = (episode2[:N] == episode).cpu()  # (`fresh` numbers the episodes by env id: the same for both populations)
    assert same_episode.all() and torch.equal(state2[:N], state), name
    # a different episode or seed gives a different row
    again = state.clone()
    reset_fn(name, SEED, ascending, None, again, steps, episode, max_steps)
    assert not torch.equal(again[:, 0], state[:, 0]), name
    state3, steps3, episode3 = fresh(name, N, device)
    reset_fn(name, SEED + 1, ascending, None, state3, steps3, episode3, max_steps)
    assert not torch.equal(state3[:, 0], state[:, 0]), name
    out["all"] = (state.cpu(), again.cpu(), state3.cpu())
    # randomize_progress: steps in [0, max_steps), not constant at N = 257
    state4, steps4, episode4 = fresh(name, N, device)
    reset_fn(name, SEED, ascending, None, state4, steps4, episode4, max_steps, True)
    assert ((steps4 >= 0) & (steps4 < max_steps)).all() and torch.equal(state4, state), name
    if N == 257:
        assert steps4.unique().numel() > 16, name
    out["progress"] = (steps4.cpu(),)
    return out
