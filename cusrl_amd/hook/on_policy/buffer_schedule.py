"""Rollout length on a schedule (counterpart of cusrl/hook/on_policy/buffer_schedule.py).

Runs in ``apply_schedule``, between two iterations.  A new capacity empties and re-allocates the buffer
(``Buffer.resize``), which moves ``Buffer.layout_version``: every captured region sized by the rollout length — the env
steps, the value pass, the statistics pass, the minibatch steps — is captured again, once, and replays while the capacity
holds (template/graphs.py)."""

from __future__ import annotations

from collections.abc import Callable

from cusrl_amd.template.hook import Hook

__all__ = ["OnPolicyBufferCapacitySchedule"]


class OnPolicyBufferCapacitySchedule(Hook):
    """Sets ``agent.num_steps_per_update`` and the buffer's capacity to ``schedule(iteration)``."""

    def __init__(self, schedule: Callable[[int], int]):
        super().__init__(training_only=True)
        self.schedule = schedule

    def apply_schedule(self, iteration: int):
        capacity = self.schedule(iteration)
        self.agent.num_steps_per_update = capacity
        self.agent.resize_buffer(capacity)
