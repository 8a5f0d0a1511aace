"""State estimation (counterpart of cusrl/hook/auxiliary/estimation.py:13-131): a dedicated estimator reads a slice of one
transition entry during the rollout, its output is stored in the transition, and it is trained with an MSE loss against a
slice of another entry — typically privileged state reconstructed from observations.  The estimator stays a torch module;
its loss and ``d loss / d estimation`` are one HIP launch with the target leaf read in place
(``cusrl_column_mse_fwd_bwd``, hook/auxiliary/_column_mse.py).

Not here: recurrent estimators (their ``estimator_memory`` leaf and temporal batches have no device form yet)."""

from __future__ import annotations

import torch
from torch import nn

from cusrl_amd.hook.auxiliary._column_mse import ColumnSelection, weighted_column_mse
from cusrl_amd.template.hook import Hook

__all__ = ["StateEstimation"]


class StateEstimation(Hook):
    """Learns an auxiliary estimator between transition entries.

    Args:
        estimator_factory:
            Factory of the estimator module; it receives the sliced source and target dimensions.
        source_name (str):
            Transition key used as the estimator input. Defaults to ``"observation"``.
        source_indices (Slice):
            Slice applied to ``source_name`` before passing it to the estimator. Defaults to ``slice(None)``.
        source_dim (int | None):
            Full dimension of ``source_name`` before slicing; inferred for ``"observation"``, ``"next_observation"``,
            ``"state"`` and ``"next_state"`` when omitted.
        target_name (str):
            Transition key used as the supervision target. Defaults to ``"state"``.
        target_indices (Slice):
            Slice applied to ``target_name`` before computing the loss. Defaults to ``slice(None)``.
        target_dim (int | None):
            Full dimension of ``target_name`` before slicing; inferred like ``source_dim``.
        estimation_name (str):
            Transition key the estimator output is stored under during rollout. Defaults to ``"state_estimation"``.
        weight (float):
            Multiplicative weight of the state estimation loss. Defaults to ``1.0``.
    """

    rollout_capture_safe = True

    def __init__(self, estimator_factory, source_name: str = "observation", source_indices=slice(None),
                 source_dim: int | None = None, target_name: str = "state", target_indices=slice(None),
                 target_dim: int | None = None, estimation_name: str = "state_estimation", weight: float = 1.0):
        super().__init__()
        self.estimator_factory = estimator_factory
        self.source_name = source_name
        self.source_indices = source_indices
        self.source_dim = source_dim
        self.target_name = target_name
        self.target_indices = target_indices
        self.target_dim = target_dim
        self.estimation_name = estimation_name

        # Mutable attributes
        self.weight: float = weight
        self.register_mutable("weight")

        # Runtime attributes
        self.estimator: nn.Module
        self.criterion: nn.MSELoss
        self._estimator_memory = None

    def _infer_dim(self, name: str, which: str) -> int:
        if name == "observation" or name == "next_observation":
            return self.agent.observation_dim
        if name == "state" or name == "next_state":
            return self.agent.state_dim
        raise ValueError(f"'{which}_dim' must be specified for {which}_name '{name}'.")

    def init(self):
        if self.source_dim is None:
            self.source_dim = self._infer_dim(self.source_name, "source")
        if self.target_dim is None:
            self.target_dim = self._infer_dim(self.target_name, "target")

        source_dim = torch.zeros(1, self.source_dim)[..., self.source_indices].numel()
        self._target = ColumnSelection(self.target_indices, self.target_dim)
        estimator = self.estimator_factory(source_dim, self._target.dim)
        if getattr(estimator, "is_recurrent", False):
            raise NotImplementedError(
                f"{type(self).__name__} does not support recurrent estimators yet: the 'estimator_memory' leaf and temporal "
                "batches of the reference have no device form here")
        self.register_module("estimator", estimator.rnn_compatible())
        self.criterion = nn.MSELoss()
        self._target.prepare(self.agent.device)  # the column table is uploaded now, outside any capture

    @property
    def post_step_device_free(self) -> bool:
        return self._estimator_memory is None  # a feed-forward estimator has no memory to reset

    def pre_act(self, transition):
        source = transition[self.source_name][..., self.source_indices]
        estimation, next_estimator_memory = self.estimator(source, memory=self._estimator_memory, sequential=False)

        transition[self.estimation_name] = estimation
        transition["estimator_memory"] = self._estimator_memory  # None (feed-forward): the buffer stores no such leaf
        self._estimator_memory = next_estimator_memory

    def post_step(self, transition):
        self.estimator.reset_memory(self._estimator_memory, transition["done"])

    def export_stages(self, which: str = "actor"):
        # pre_act writes the estimate beside the observation: the actor's input is untouched unless it is stored over it
        if self.estimation_name == "observation":
            raise ValueError(f"ActorCritic.export: hook '{self.name}' stores its estimate as the actor's observation; no export "
                             "stage expresses an estimator in front of the actor")
        return ()

    def objective(self, metadata, batch):
        source = batch[self.source_name][..., self.source_indices]
        estimation, _ = self.estimator(source, memory=batch.get("estimator_memory"), done=batch["done"])
        loss = weighted_column_mse(type(self).__name__, self.criterion, estimation, batch[self.target_name], self._target,
                                   self.weight)
        return {"state_estimation_loss": loss}
