"""Schedules over another hook's mutable attribute or activity flag (counterpart of cusrl/hook/control/schedule.py).

Both run in ``apply_schedule`` — between two iterations, never inside a captured region.  What they change is part of
``graphs.capture_signature``: a graph captured under the old value is not replayed, and a region whose signature keeps
changing stays eager instead of capturing every iteration (template/graphs.py)."""

from __future__ import annotations

from collections.abc import Callable
from typing import Any

from cusrl_amd.template.hook import Hook

__all__ = ["HookActivationSchedule", "HookParameterSchedule"]


class _NamedHookSchedule(Hook):
    hook_name: str

    def init(self):
        try:
            self.agent.hook[self.hook_name]
        except KeyError:
            raise ValueError(f"No hook named '{self.hook_name}' is registered") from None


class HookParameterSchedule(_NamedHookSchedule):
    """Sets ``parameter`` of the hook ``hook_name`` to ``scheduler(iteration)`` through ``Hook.update_attribute`` (the
    attribute must be a registered mutable); float values are also recorded as the metric ``{hook_name}_{parameter}``."""

    def __init__(self, hook_name: str, parameter: str, scheduler: Callable[[int], Any]):
        super().__init__(training_only=True)
        self.hook_name = hook_name
        self.parameter = parameter
        self.scheduler = scheduler
        self.name_(f"{hook_name}_{parameter}_schedule")

    def apply_schedule(self, iteration: int):
        value = self.scheduler(iteration)
        self.agent.hook[self.hook_name].update_attribute(self.parameter, value)
        if isinstance(value, float):
            self.agent.record(**{f"{self.hook_name}_{self.parameter}": value})


class HookActivationSchedule(_NamedHookSchedule):
    """Switches the hook ``hook_name`` on or off: ``active_(scheduler(iteration))``."""

    def __init__(self, hook_name: str, scheduler: Callable[[int], bool]):
        super().__init__(training_only=True)
        self.hook_name = hook_name
        self.scheduler = scheduler
        self.name_(f"{hook_name}_activation_schedule")

    def apply_schedule(self, iteration: int):
        self.agent.hook[self.hook_name].active_(self.scheduler(iteration))
