"""What tests/test_classic_control.py (host form) and tests/test_classic_control_gpu.py (kernels) share for the five tasks: the
input tables, a float64 evaluation of the tasks' TEXTBOOK formulas written independently of the C body (Acrobot: ``cos(x - pi/2)``,
unfolded constants, a looped wrap, where the C body folds the constants and wraps in closed form), the error measure, and the
reset cases.

Error measure (``scaled_error``): ``max |got - ref| / max(1, |ref|)`` over the new state, the observation and the reward — the
tasks' quantities are O(1) .. O(10), so this is "ulps of the largest operand" up to a factor below 2.

``HOST_ERROR`` is the largest error of the library's host restatement against the float64 evaluation on these inputs, measured
on the build machine (x86-64, glibc's sinf / cosf / sincosf) and written into DESIGN.md §7; the CPU test asserts it with a factor
2, the GPU test with a factor 4 (the device's sinf / cosf are not glibc's): the project's established margins."""

from __future__ import annotations

import numpy as np
import torch

ACROBOT, CONTINUOUS = "Acrobot-v1", "MountainCarContinuous-v0"
TASKS = {"CartPole": dict(S=4, A=2, O=4, max_steps=500), "Pendulum": dict(S=2, A=1, O=3, max_steps=200),
         "MountainCar": dict(S=2, A=3, O=2, max_steps=200), ACROBOT: dict(S=4, A=3, O=6, max_steps=500),
         CONTINUOUS: dict(S=2, A=1, O=2, max_steps=999)}
# measured with tests/test_classic_control.py::test_host_restatement_against_float64 (it prints each figure before it asserts)
HOST_ERROR = {"CartPole": 1.1e-7, "Pendulum": 4.7e-7, "MountainCar": 5.5e-8,  # measured 1.080e-7, 4.660e-7, 5.403e-8,
              ACROBOT: 6.0e-6, CONTINUOUS: 5.4e-8}  # 5.908e-6, 5.343e-8
TRIG_COLUMNS = {"Pendulum": 2, ACROBOT: 4}  # the leading observation columns that are cos, sin of the leading state columns
RANDOM_ROWS = 257
PI = np.pi

_F = np.float32(-1.2)  # (the clamp's own fp32 value: the tables need a position that IS the saturated one)

# Per task: the fixed table (a row: the S state columns, the action, the step counter), then what the random rows draw
TABLES = {
    "CartPole": [  # x, x', theta, theta', logits, steps
        (0.0, 0.0, 0.0, 0.0, (0, 1), 0), (0.0, 0.0, 0.0, 0.0, (1, 0), 0),
        (0.01, -0.02, 0.03, 0.04, (0, 0), 3),  # tie: column 0
        (0.01, -0.02, 0.03, 0.04, (1, 1), 3), (-0.5, 1.0, -0.1, 0.5, (0.3, 0.7), 10), (1.0, -1.5, 0.15, -1.0, (-1, -2), 10),
        (2.39, 2.0, 0.0, 0.0, (0, 1), 20),  # leaves the track on the right
        (-2.395, -1.0, 0.05, 0.0, (1, 0), 20), (0.0, 0.0, 0.2, 1.5, (0, 1), 20),  # falls over
        (0.0, 0.0, -0.205, -1.0, (1, 0), 499),  # terminated at the step limit: not truncated
        (2.3, 0.5, 0.0, 0.1, (0, 1), 499),  # survives at the step limit: truncated
        (0.2, 0.1, 0.05, 0.0, (0, 1), 498),  # one short of it
    ],
    "Pendulum": [  # theta, theta', torque, steps
        (0.0, 0.0, 0.0, 0), (0.5, 1.0, 1.0, 5), (3.1, -1.0, 2.0, 5), (-3.1, 1.0, -2.0, 5),
        (3.5, 0.5, 0.3, 7), (-3.5, -0.5, -0.3, 7),  # outside (-pi, pi] on both sides
        (7.0, 2.0, 0.0, 7), (-7.0, -2.0, 0.0, 7), (10.0, 0.0, 1.0, 7), (-10.0, 0.0, -1.0, 7),
        (1.0, 8.0, 2.0, 9), (-1.0, -8.0, -2.0, 9),  # |theta'| = 8 pushed further: the clamp saturates
        (1.0, 7.9, 2.5, 9), (-1.0, -7.9, -2.5, 9),  # |a| > 2 and the clamp of theta'
        (0.3, 0.0, 3.0, 9), (0.3, 0.0, -3.0, 9), (0.3, 0.0, 2.0, 9),  # |a| > 2 alone gives what a = 2 gives
        (2.0, 1.0, 0.5, 199), (2.0, 1.0, 0.5, 198),  # truncated at the step limit / one short of it
    ],
    "MountainCar": [  # position, velocity, logits, steps
        (_F, -0.01, (1, 0, 0), 0),  # at the left wall moving left: velocity zeroed
        (_F, 0.02, (0, 0, 1), 0), (-0.5, 0.07, (0, 0, 1), 4), (-0.5, -0.07, (1, 0, 0), 4),  # v = +-0.07 pushed further
        (0.6, 0.05, (0, 0, 1), 4),  # p = 0.6 pushed further; terminated
        (0.48, 0.03, (0, 1, 0), 4),  # crosses 0.5
        (0.45, 0.03, (0, 1, 0), 4),  # does not
        (-0.5, 0.0, (0, 0, 0), 6),  # ties: column 0
        (-0.5, 0.0, (1, 2, 2), 6),  # column 1
        (-0.5, 0.0, (5, 1, 5), 6),  # column 0
        (-0.3, 0.01, (0, 0.5, 0.25), 199),  # truncated at the step limit
        (0.49, 0.05, (0, 0, 1), 199),  # terminated at the step limit: not truncated
        (-0.3, 0.01, (0, 1, 0), 198),
    ],
    ACROBOT: [  # theta1, theta2, theta1', theta2', logits, steps
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
    ],
    CONTINUOUS: [  # position, velocity, action, steps
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
    ],
}
_ON_THE_TRACK = lambda rng, M: rng.uniform(0, 1, (M, 2)) * np.array([1.8, 0.14]) + np.array([-1.2, -0.07])  # noqa: E731
RANDOM = {  # name: (seed, the state rows, the action rows), drawn in this order
    "CartPole": (11, lambda rng, M: rng.uniform(-1, 1, (M, 4)) * np.array([2.4, 2.0, 0.2095, 2.0]),
                 lambda rng, M: rng.randint(0, 2, (M, 2))),  # (ties included)
    "Pendulum": (12, lambda rng, M: rng.uniform(-1, 1, (M, 2)) * np.array([np.pi, 8.0]), lambda rng, M: rng.uniform(-2.5, 2.5, (M, 1))),
    "MountainCar": (13, _ON_THE_TRACK, lambda rng, M: rng.randint(0, 2, (M, 3))),
    ACROBOT: (14, lambda rng, M: rng.uniform(-1, 1, (M, 4)) * np.array([PI, PI, 4 * PI, 9 * PI]),
              lambda rng, M: rng.randint(0, 2, (M, 3))),  # (ties included)
    CONTINUOUS: (15, _ON_THE_TRACK, lambda rng, M: rng.uniform(-1.5, 1.5, (M, 1))),
}


def inputs(name: str):
    """``(state [M, S] fp32, action [M, A] fp32, steps [M] int32, max_steps)``: the fixed table, then 257 seeded random rows."""
    S, M, max_steps = TASKS[name]["S"], RANDOM_ROWS, TASKS[name]["max_steps"]
    table, (seed, draw_state, draw_action) = TABLES[name], RANDOM[name]
    rng = np.random.RandomState(seed)
    state = np.array([row[:S] for row in table], dtype=np.float32)
    action = np.array([np.atleast_1d(row[S]) for row in table], dtype=np.float32)
    steps = np.array([row[S + 1] for row in table], dtype=np.int32)
    random_state = draw_state(rng, M)
    random_action = draw_action(rng, M)
    random_steps = rng.randint(0, max_steps, M)
    random_steps[:4] = max_steps - 1
    state = np.concatenate([state, random_state.astype(np.float32)])
    action = np.concatenate([action, random_action.astype(np.float32)])
    steps = np.concatenate([steps, random_steps.astype(np.int32)])
    return torch.from_numpy(state), torch.from_numpy(action), torch.from_numpy(steps), max_steps


# ------------------------------------------------------------------------------------------------ the tasks in float64
# Each: (s [M, S], a [M, A], saturated [M, S] to fill in) -> dict(state, observation, reward, terminated, margin[, raw])
def _cartpole(s, a, saturated):
    x, x_dot, theta, theta_dot = s.T
    force = np.where(np.argmax(a, axis=1) == 1, 10.0, -10.0)
    g, m_cart, m_pole, length, tau = 9.8, 1.0, 0.1, 0.5, 0.02
    total = m_cart + m_pole
    sin, cos = np.sin(theta), np.cos(theta)
    temp = (force + m_pole * length * theta_dot**2 * sin) / total
    theta_acc = (g * sin - cos * temp) / (length * (4.0 / 3.0 - m_pole * cos**2 / total))
    x_acc = temp - m_pole * length * theta_acc * cos / total
    new = np.stack([x + tau * x_dot, x_dot + tau * x_acc, theta + tau * theta_dot, theta_dot + tau * theta_acc], axis=1)
    limit = 12 * 2 * np.pi / 360
    terminated = (np.abs(new[:, 0]) > 2.4) | (np.abs(new[:, 2]) > limit)
    margin = np.minimum(np.abs(np.abs(new[:, 0]) - 2.4) / 2.4, np.abs(np.abs(new[:, 2]) - limit))
    return dict(state=new, observation=new.copy(), reward=np.ones(s.shape[0]), terminated=terminated, margin=margin)


def _pendulum(s, a, saturated):
    theta, theta_dot = s.T
    u = np.clip(a[:, 0], -2.0, 2.0)
    wrapped = np.mod(theta + np.pi, 2 * np.pi) - np.pi
    reward = -(wrapped**2 + 0.1 * theta_dot**2 + 0.001 * u**2)
    g, m, length, dt = 10.0, 1.0, 1.0, 0.05
    raw = theta_dot + (3 * g / (2 * length) * np.sin(theta) + 3.0 / (m * length**2) * u) * dt
    new_dot = np.clip(raw, -8.0, 8.0)
    saturated[:, 1] = np.abs(raw) > 8.0
    new_theta = theta + new_dot * dt
    observation = np.stack([np.cos(new_theta), np.sin(new_theta), new_dot], axis=1)
    margin = np.abs(np.abs(raw) - 8.0) / 8.0  # (no flag to flip; `saturated` needs to know on which side of the clamp a row is)
    return dict(state=np.stack([new_theta, new_dot], axis=1), observation=observation, reward=reward,
                terminated=np.zeros(s.shape[0], dtype=bool), margin=margin)


def _mountain_car_tail(p, raw_v, goal, saturated):
    """What the two mountain cars share, from the raw velocity on -> ``(new state, terminated, margin, raw)``.  The margin's
    flips: p across the goal; v across 0 while p >= goal; the wall branch (raw p across -1.2 while moving left, or v across 0 at
    the wall); the clamps' edges."""
    clamped_v = np.clip(raw_v, -0.07, 0.07)
    raw_p = p + clamped_v
    new_p = np.clip(raw_p, -1.2, 0.6)
    wall = (new_p == -1.2) & (clamped_v < 0)
    saturated[:, 1] = (np.abs(raw_v) > 0.07) | wall
    saturated[:, 0] = (raw_p < -1.2) | (raw_p > 0.6)
    new_v = np.where(wall, 0.0, clamped_v)
    terminated = (new_p >= goal) & (new_v >= 0)
    margin = np.abs(new_p - goal)
    margin = np.minimum(margin, np.where(new_p >= goal, np.abs(new_v), np.inf))
    margin = np.minimum(margin, np.where(clamped_v < 0, np.abs(raw_p + 1.2) / 1.2, np.inf))
    margin = np.minimum(margin, np.where(raw_p <= -1.2, np.abs(clamped_v), np.inf))
    margin = np.minimum(margin, np.minimum(np.abs(np.abs(raw_v) - 0.07), np.minimum(np.abs(raw_p + 1.2) / 1.2, np.abs(raw_p - 0.6))))
    return np.stack([new_p, new_v], axis=1), terminated, margin, np.stack([raw_p, raw_v], axis=1)


def _mountain_car(s, a, saturated):
    p, v = s.T
    push = np.argmax(a, axis=1)
    new, terminated, margin, raw = _mountain_car_tail(p, v + (push - 1) * 0.001 - 0.0025 * np.cos(3 * p), 0.5, saturated)
    return dict(state=new, observation=new.copy(), reward=-np.ones(s.shape[0]), terminated=terminated, margin=margin, raw=raw)


def _mountain_car_continuous(s, a, saturated):
    """(The force clamp is continuous, flips nothing and leaves no constant in the state: it has no margin, so the table may hold
    a = +-1 itself.)"""
    p, v = s.T
    force = np.clip(a[:, 0], -1.0, 1.0)
    new, terminated, margin, raw = _mountain_car_tail(p, v + (force * 0.0015 - 0.0025 * np.cos(3 * p)), 0.45, saturated)
    reward = np.where(terminated, 100.0, 0.0) - 0.1 * a[:, 0] ** 2  # the RAW action
    return dict(state=new, observation=new.copy(), reward=reward, terminated=terminated, margin=margin, raw=raw)


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


def _acrobot(s, a, saturated):
    """Margin: the termination line, the raw angles against every odd multiple of pi, the raw velocities against 4 pi and 9 pi."""
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
    return dict(state=new, observation=observation, reward=reward, terminated=terminated, margin=margin, raw=raw)


_FLOAT64 = {"CartPole": _cartpole, "Pendulum": _pendulum, "MountainCar": _mountain_car, ACROBOT: _acrobot,
            CONTINUOUS: _mountain_car_continuous}


def reference_step(name: str, state: torch.Tensor, action: torch.Tensor, steps: torch.Tensor, max_steps: int) -> dict:
    """The task's formulas in float64 from the fp32 inputs.  ``margin``: per row, how far the float64 result sits from the nearest
    threshold at which a flag or a discontinuous branch flips or a clamp starts to hold, in units of ``max(1, |threshold|)``.
    ``saturated``: the entries of the new state that are a clamp's bound (or the zeroed velocity) — constants, whatever the
    rounding before them.  ``raw`` (the mountain cars, Acrobot): the new state before its clamps and wrap."""
    s, a = state.numpy().astype(np.float64), action.numpy().astype(np.float64)
    saturated = np.zeros_like(s, dtype=bool)
    out = _FLOAT64[name](s, a, saturated)
    new_steps = steps.numpy().astype(np.int64) + 1
    terminated = out.pop("terminated")
    truncated = (new_steps >= max_steps) & ~terminated
    assert out["margin"].shape == (s.shape[0],)
    return dict(out, reward=out["reward"][:, None], terminated=terminated[:, None], truncated=truncated[:, None], steps=new_steps,
                saturated=saturated)


def scaled_error(got, ref: np.ndarray) -> float:
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0


def step_error(result: dict, reference: dict) -> float:
    """The largest ``scaled_error`` over new state, observation and reward of one ``classic_step`` result."""
    return max(scaled_error(result[key], reference[key]) for key in ("state", "observation", "reward"))


def assert_exact_parts(result: dict, reference: dict, name: str):
    """Flags and the step counter exactly as the float64 evaluation gives them."""
    for key in ("terminated", "truncated"):
        assert np.array_equal(result[key].cpu().numpy(), reference[key]), (name, key)
    assert np.array_equal(result["steps"].cpu().numpy().astype(np.int64), reference["steps"]), name


def run_step(step_fn, name: str, state, action, steps, max_steps) -> dict:
    """``step_fn`` = ``ops.classic_step`` or ``ops.classic_step_cpu`` on copies of the inputs -> everything it produced."""
    state, steps = state.clone(), steps.clone()
    observation, reward, terminated, truncated = step_fn(name, action, state, steps, max_steps)
    return dict(state=state, observation=observation, reward=reward, terminated=terminated, truncated=truncated, steps=steps)


# ------------------------------------------------------------------------------------------------------------------- reset
RANGES = {"CartPole": [(-0.05, 0.05)] * 4, "Pendulum": [(-np.pi, np.pi), (-1.0, 1.0)], "MountainCar": [(-0.6, -0.4), (0.0, 0.0)],
          ACROBOT: [(-0.1, 0.1)] * 4, CONTINUOUS: [(-0.6, -0.4), (0.0, 0.0)]}
SEED = 0x1234_5678_9ABC_DEF0


def fresh(name: str, N: int, device):
    """A marked, non-zero env state: rows that a reset must not touch are recognisable."""
    S = TASKS[name]["S"]
    state = (torch.arange(N * S, dtype=torch.float32).reshape(N, S) * 0.001 + 0.3).to(device)
    steps = (torch.arange(N, dtype=torch.int32) % 50 + 7).to(device)
    episode = (torch.arange(N, dtype=torch.int64) % 5 + 2).to(device)
    return state, steps, episode


def observation_of(name: str, state: torch.Tensor) -> np.ndarray:
    """cos, sin of each leading angle (``TRIG_COLUMNS``), then the remaining state columns; float64."""
    s = state.cpu().numpy().astype(np.float64)
    angles = TRIG_COLUMNS.get(name, 0) // 2
    trig = [f(s[:, j]) for j in range(angles) for f in (np.cos, np.sin)]
    return np.stack(trig + [s[:, j] for j in range(angles, s.shape[1])], axis=1)


def assert_observation(name: str, observation: torch.Tensor, state_rows: torch.Tensor, bound: float, where):
    """An observation row is its state row: the bits of every column that is a state column (all of CartPole's and the mountain
    cars', Pendulum's theta', Acrobot's two velocities), within ``bound`` of the float64 cos / sin of the fp32 angles for
    Pendulum's first two and Acrobot's first four columns."""
    trig = TRIG_COLUMNS.get(name, 0)
    assert torch.equal(observation[:, trig:].cpu(), state_rows[:, trig // 2 :].cpu()), where
    if trig:
        assert scaled_error(observation, observation_of(name, state_rows)) <= bound, where


def reset_cases(reset_fn, name: str, device, N: int) -> dict:
    """Every reset case through ``reset_fn`` (``ops.classic_reset`` / ``ops.classic_reset_cpu``) on ``device``; asserts the
    properties and returns the produced tensors (on the CPU) so that two devices can be compared."""
    max_steps = TASKS[name]["max_steps"]
    bound = 4 * HOST_ERROR[name]
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
