"""Hooks that edit the agent's ``environment_spec`` before anything is built from it (counterparts of
cusrl/hook/mdp/environment_spec.py:10-59).  Host-only: they run once, in ``pre_init``, ahead of the networks, the buffer and
every other hook's ``init``."""

from __future__ import annotations

from collections.abc import Callable
from typing import Any

from cusrl_amd.template.hook import Hook

__all__ = ["DynamicEnvironmentSpecOverride", "EnvironmentSpecOverride"]


def _apply(spec, overrides: dict[str, Any]):
    for key, value in overrides.items():
        setattr(spec, key, value)


class EnvironmentSpecOverride(Hook):
    """Sets the given attributes on ``agent.environment_spec``; a dict and keyword arguments are merged (keywords win)."""

    def __init__(self, overrides: dict[str, Any] | None = None, **kwargs):
        super().__init__()
        self.overrides = {**(overrides or {}), **kwargs}

    def pre_init(self, agent):
        super().pre_init(agent)
        _apply(agent.environment_spec, self.overrides)


class DynamicEnvironmentSpecOverride(Hook):
    """The same with overrides computed from the live environment: ``overrides_factory(environment_instance)``."""

    def __init__(self, overrides_factory: Callable[[Any], dict[str, Any]]):
        super().__init__()
        self.overrides_factory = overrides_factory

    def pre_init(self, agent):
        super().pre_init(agent)
        instance = agent.environment_spec.environment_instance
        if instance is None:
            raise ValueError("'environment_instance' is not set in the environment_spec")
        _apply(agent.environment_spec, self.overrides_factory(instance))
