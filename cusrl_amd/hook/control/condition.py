"""Objective hooks switched on and off per minibatch step (counterpart of cusrl/hook/control/condition.py).

Capture policy: a condition is an arbitrary callable of ``(agent, metadata, batch)`` evaluated on the host in front of every
minibatch step, and it flips activity flags the step's other hooks are then dispatched by.  A replayed hipGraph runs no Python,
so the flip cannot live inside a captured step, and a key over the activity pattern would need the condition's answer before the
step's batch exists.  The hook therefore declares the objective phase eager (``Hook.eager_phases``): the minibatch steps of an
agent that uses it run hook by hook, everything outside them (rollout, value pass, statistics) stays captured."""

from __future__ import annotations

from collections.abc import Callable, Iterable
from typing import Any

from cusrl_amd.template.hook import Hook

__all__ = ["ConditionalObjectiveActivation", "EpochIndexCondition"]

ActivationCondition = Callable[[Any, dict[str, Any], dict[str, Any]], bool]


class EpochIndexCondition:
    """True in the epochs listed (one index or several)."""

    def __init__(self, epoch_index: int | Iterable[int]):
        self.epoch_index = {epoch_index} if isinstance(epoch_index, int) else set(epoch_index)

    def __call__(self, agent, metadata: dict[str, Any], batch: dict[str, Any]) -> bool:
        return metadata["epoch_index"] in self.epoch_index


class ConditionalObjectiveActivation(Hook):
    """Activates the named objective hooks only in the minibatch steps their condition holds for.  Must stand in front of the
    hooks it controls.

    Args:
        named_conditions (dict[str, ActivationCondition] | None) / keyword arguments:
            hook name -> ``condition(agent, metadata, batch) -> bool``.  A hook that was inactive when the update began stays
            inactive whatever its condition says, and every hook has its earlier activity back after the update.
    """

    def __init__(self, named_conditions: dict[str, ActivationCondition] | None = None, **kwargs: ActivationCondition):
        super().__init__(training_only=True)
        self.named_conditions = {**(named_conditions or {}), **kwargs}
        self._named_activation: dict[str, bool] = {}

    def eager_phases(self) -> tuple[str, ...]:
        return ("objective",)

    def pre_update(self, buffer):
        for name in self.named_conditions:
            self._named_activation[name] = self.agent.hook[name].active

    def pre_objective(self, metadata, batch):
        for name, condition in self.named_conditions.items():
            holds = condition(self.agent, metadata, batch)
            self.agent.hook[name].active_(self._named_activation[name] and holds)

    def post_update(self):
        for name in self.named_conditions:
            self.agent.hook[name].active_(self._named_activation[name])
