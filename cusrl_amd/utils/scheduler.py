"""Iteration-indexed callables for the schedule hooks (counterpart of cusrl/utils/scheduler.py): ``scheduler(iteration)`` is the
value a ``HookParameterSchedule`` / ``HookActivationSchedule`` / ``OnPolicyBufferCapacitySchedule`` applies before that
iteration.  Plain host arithmetic in Python floats — the expressions are evaluated in the reference's order, so the values are
the reference's bit for bit (tests/golden/control_hooks.npz)."""

from __future__ import annotations

import math
from typing import Any

__all__ = ["CosineAnnealingScheduler", "LessThan", "NotLessThan", "PiecewiseLinearScheduler", "StepScheduler", "TanhScheduler"]


def _check_steps(points) -> None:
    steps = [step for step, _ in points]
    for earlier, later in zip(steps, steps[1:]):
        if earlier >= later:
            raise ValueError("step coordinates must be strictly increasing")


class LessThan:
    """``iteration < threshold``."""

    def __init__(self, threshold: int):
        self.threshold = threshold

    def __call__(self, value: int) -> bool:
        return value < self.threshold


class NotLessThan:
    """``iteration >= threshold``."""

    def __init__(self, threshold: int):
        self.threshold = threshold

    def __call__(self, value: int) -> bool:
        return value >= self.threshold


class StepScheduler:
    """``initial_value`` until the first transition; from ``step`` of a transition ``(step, value)`` on, that ``value`` (any
    type).  Steps strictly increasing."""

    def __init__(self, initial_value: Any, *transitions: tuple[int, Any]):
        self.initial_value = initial_value
        self.transitions = transitions
        _check_steps(transitions)

    def __call__(self, iteration: int) -> Any:
        current = self.initial_value
        for step, value in self.transitions:
            if iteration < step:
                return current
            current = value
        return current


class PiecewiseLinearScheduler:
    """Linear between consecutive anchors ``(step, value)``, constant in front of the first and behind the last.  At least
    two anchors, steps strictly increasing."""

    def __init__(self, *anchors: tuple[int, float]):
        if len(anchors) < 2:
            raise ValueError("at least two anchors are required")
        self.anchors = anchors
        _check_steps(anchors)

    def __call__(self, iteration: int) -> float:
        if iteration <= self.anchors[0][0]:
            return self.anchors[0][1]
        for (step0, value0), (step1, value1) in zip(self.anchors, self.anchors[1:]):
            if iteration <= step1:
                return value0 + (value1 - value0) * ((iteration - step0) / (step1 - step0))
        return self.anchors[-1][1]


class CosineAnnealingScheduler:
    """Half a cosine from ``start = (step, value)`` to ``end = (step, value)``, constant outside."""

    def __init__(self, start: tuple[int, float], end: tuple[int, float]):
        self.start_step, self.start_value = start
        self.end_step, self.end_value = end
        _check_steps((start, end))

    def __call__(self, iteration: int) -> float:
        if iteration <= self.start_step:
            return self.start_value
        if iteration >= self.end_step:
            return self.end_value
        ratio = (iteration - self.start_step) / (self.end_step - self.start_step)
        return self.end_value + 0.5 * (self.start_value - self.end_value) * (1 + math.cos(math.pi * ratio))


class TanhScheduler:
    """A tanh-shaped transition from ``start`` to ``end`` (``eta > 0``: its steepness), rescaled so that both anchors are hit
    exactly; constant outside."""

    def __init__(self, start: tuple[int, float], end: tuple[int, float], eta: float):
        self.start_step, self.start_value = start
        self.end_step, self.end_value = end
        self.eta = eta
        _check_steps((start, end))
        if self.eta <= 0:
            raise ValueError("'eta' must be positive")
        self.mid_step = (self.start_step + self.end_step) / 2
        self.start_epsilon = self._get_epsilon(self.start_step)
        self.end_epsilon = self._get_epsilon(self.end_step)

    def _get_epsilon(self, iteration: int) -> float:
        return 0.5 + 0.5 * math.tanh(self.eta * (2 * (iteration - self.mid_step) / (self.end_step - self.start_step)))

    def __call__(self, iteration: int) -> float:
        if iteration <= self.start_step:
            return self.start_value
        if iteration >= self.end_step:
            return self.end_value
        ratio = (self._get_epsilon(iteration) - self.start_epsilon) / (self.end_epsilon - self.start_epsilon)
        return self.start_value + (self.end_value - self.start_value) * ratio
