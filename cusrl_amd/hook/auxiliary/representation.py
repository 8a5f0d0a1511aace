"""Representation objectives on the actor's latent (counterpart of cusrl/hook/auxiliary/representation.py:13-182): a small
predictor on ``actor.intermediate_repr[latent_name]`` is trained to predict the return (or value), a slice of the privileged
state, or — given the action — a slice of the next state, which makes the latent encode them.  The predictors stay torch
modules; each loss with its ``d loss / d prediction`` is one HIP launch with the target leaf of the minibatch read in place
(``cusrl_column_mse_fwd_bwd``, hook/auxiliary/_column_mse.py).

Not here: ``post_export`` (export is out of scope)."""

from __future__ import annotations

import torch
from torch import nn

from cusrl_amd.hook.auxiliary._column_mse import ColumnSelection, weighted_column_mse
from cusrl_amd.template.hook import Hook

__all__ = ["ActionAwarePredictorWrapper", "NextStatePrediction", "ReturnPrediction", "StatePrediction"]


class _LatentHook(Hook):
    latent_name: str

    def _latent_dim(self) -> int:
        """Width of the latent, probed like the reference does: one forward of the actor on a zero observation.  The actor's
        no-grad pass is fused into one launch that records no latent (``Actor.fused_inference``): switched off for the probe."""
        actor = self.agent.actor
        fused, actor.fused_inference = actor.fused_inference, False
        try:
            with torch.no_grad():
                actor(torch.zeros(1, self.agent.observation_dim, device=actor.device))
            return actor.intermediate_repr[self.latent_name].numel()
        finally:
            actor.fused_inference = fused
            actor.clear_intermediate_repr()

    def _latent(self):
        return self.agent.actor.intermediate_repr[self.latent_name]


class ReturnPrediction(_LatentHook):
    def __init__(self, latent_name: str = "backbone.output", weight: float = 0.01, predictor_factory=nn.Linear,
                 predicts_value_instead_of_return: bool = False):
        super().__init__()
        self.latent_name = latent_name
        self.predictor_factory = predictor_factory
        self.predicts_value_instead_of_return = predicts_value_instead_of_return

        # Mutable attributes
        self.weight: float = weight
        self.register_mutable("weight")

        # Runtime attributes
        self.predictor: nn.Module
        self.criterion: nn.MSELoss

    def init(self):
        self.register_module("predictor", self.predictor_factory(self._latent_dim(), self.agent.value_dim))
        self.criterion = nn.MSELoss()

    def objective(self, metadata, batch):
        target = batch["value"] if self.predicts_value_instead_of_return else batch["return"]
        prediction = self.predictor(self._latent())
        loss = weighted_column_mse(type(self).__name__, self.criterion, prediction, target, None, self.weight)
        return {"return_prediction_loss": loss}


class StatePrediction(_LatentHook):
    """A hook to predict states from actor representations.

    This hook adds an auxiliary loss to the main training objective: the MSELoss between the predicted state and the actual
    state, which encourages the specified latent representation to encode information about states (or privileged
    information).

    Args:
        target_indices (Slice):
            Indices of the state to be predicted.
        latent_name (str):
            The name of the intermediate representation from the actor to be used as input of the predictor. Defaults to
            ``"backbone.output"``.
        weight (float):
            The weight of the state prediction loss in the total objective. Defaults to ``0.01``.
        predictor_factory:
            A callable that creates the predictor module (e.g., `nn.Linear`). Defaults to ``nn.Linear``.
    """

    def __init__(self, target_indices, latent_name: str = "backbone.output", weight: float = 0.01, predictor_factory=nn.Linear):
        super().__init__()
        self.target_indices = target_indices
        self.latent_name = latent_name
        self.predictor_factory = predictor_factory

        # Mutable attributes
        self.weight: float = weight
        self.register_mutable("weight")

        # Runtime attributes
        self.predictor: nn.Module
        self.criterion: nn.MSELoss

    def init(self):
        if not self.agent.has_state:
            raise ValueError("StatePrediction requires the state space defined")
        self._target = ColumnSelection(self.target_indices, self.agent.state_dim)
        self.register_module("predictor", self.predictor_factory(self._latent_dim(), self._target.dim))
        self.criterion = nn.MSELoss()
        self._target.prepare(self.agent.device)  # the column table is uploaded now, outside any capture

    def objective(self, metadata, batch):
        prediction = self.predictor(self._latent())
        loss = weighted_column_mse(type(self).__name__, self.criterion, prediction, batch["state"], self._target, self.weight)
        return {"state_prediction_loss": loss}


class ActionAwarePredictorWrapper(nn.Module):
    def __init__(self, wrapped: nn.Module):
        super().__init__()
        self.wrapped = wrapped

    def forward(self, latent: torch.Tensor, action: torch.Tensor | None = None):
        if action is not None:
            latent = torch.cat([latent, action], dim=-1)
        return self.wrapped(latent)


class NextStatePrediction(_LatentHook):
    def __init__(self, target_indices, latent_name: str = "backbone.output", weight: float = 0.01, predictor_factory=nn.Linear):
        super().__init__()
        self.target_indices = target_indices
        self.latent_name = latent_name
        self.predictor_factory = predictor_factory

        # Mutable attributes
        self.weight: float = weight
        self.register_mutable("weight")

        # Runtime attributes
        self.predictor: nn.Module
        self.criterion: nn.MSELoss

    def init(self):
        if not self.agent.has_state:
            raise ValueError("NextStatePrediction requires the agent to define a state space")
        self._target = ColumnSelection(self.target_indices, self.agent.state_dim)
        predictor = self.predictor_factory(self._latent_dim() + self.agent.action_dim, self._target.dim)
        self.register_module("predictor", ActionAwarePredictorWrapper(predictor))
        self.criterion = nn.MSELoss()
        self._target.prepare(self.agent.device)  # the column table is uploaded now, outside any capture

    def objective(self, metadata, batch):
        prediction = self.predictor(self._latent(), batch["action"])
        loss = weighted_column_mse(type(self).__name__, self.criterion, prediction, batch["next_state"], self._target,
                                   self.weight)
        return {"next_state_prediction_loss": loss}
