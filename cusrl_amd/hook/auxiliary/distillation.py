"""Policy distillation loss (counterpart of cusrl/hook/auxiliary/distillation.py:12-47): the current policy mean is matched
against expert actions another component wrote into the transition.  Loss and ``d loss / d mean`` are one HIP launch
(``cusrl_column_mse_fwd_bwd`` without a column table, hook/auxiliary/_column_mse.py).

Not here: ``PolicyDistillation``, which loads a TorchScript expert and queries it at every env step."""

from __future__ import annotations

from torch import nn

from cusrl_amd.hook.auxiliary._column_mse import weighted_column_mse
from cusrl_amd.template.hook import Hook

__all__ = ["PolicyDistillationLoss"]


class PolicyDistillationLoss(Hook):
    """Matches the policy mean against precomputed expert actions.

    This hook assumes another component has already written expert actions into each transition or training batch. During
    optimization it compares the current policy mean with that target action tensor using an MSE loss.

    Args:
        target_name (str):
            Transition or batch key containing the expert action targets. Defaults to ``"expert_action"``.
        weight (float):
            Multiplicative weight applied to the distillation loss. Defaults to ``1.0``.
    """

    def __init__(self, target_name: str = "expert_action", weight: float = 1.0):
        super().__init__()
        self.target_name: str = target_name
        self.weight: float = weight
        self.register_mutable("weight")

        # Runtime attributes
        self.criterion: nn.MSELoss

    def init(self):
        self.criterion = nn.MSELoss()

    def objective(self, metadata, batch):
        mean = batch["curr_action_dist"]["mean"]
        loss = weighted_column_mse(type(self).__name__, self.criterion, mean, batch[self.target_name], None, self.weight)
        return {"distillation_loss": loss}
