"""Policy distillation loss (counterpart of cusrl/hook/auxiliary/distillation.py:12-47): the current policy mean is matched
against expert actions another component wrote into the transition.  Loss and ``d loss / d mean`` are one HIP launch
(``cusrl_column_mse_fwd_bwd`` without a column table, hook/auxiliary/_column_mse.py).

``PolicyDistillation`` (distillation.py:50-97) is that other component: it queries a frozen expert at every env step.  The
expert is a native ``nn.ExpertPolicy`` (a module, or a file in its format) or, as in the reference, a TorchScript file; only the
native one is part of a captured env step ("Distillation")."""

from __future__ import annotations

import torch
from torch import nn

from cusrl_amd.hook.auxiliary._column_mse import weighted_column_mse
from cusrl_amd.template.hook import Hook

__all__ = ["PolicyDistillation", "PolicyDistillationLoss"]


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


class PolicyDistillation(PolicyDistillationLoss):
    """Distills a pre-trained expert.

    This hook queries an expert policy on each rollout step and stores the resulting actions under ``target_name`` inherited
    from :class:`PolicyDistillationLoss`. The inherited objective then trains the current policy to match those expert actions
    with an MSE loss on the policy mean.

    The expert is treated as a recurrent policy and is reset with the transition ``"done"`` mask after each environment step
    (when it has a ``reset``).  It is no checkpointed part of the agent and receives no optimizer.

    Args:
        expert_path (str):
            Path to the expert policy: a file written by ``ExpertPolicy.save`` or by ``ActorCritic.export``, or an exported
            TorchScript module.
        observation_name (str):
            Transition key used as input to the expert policy. Defaults to ``"observation"``.
        weight (float):
            Multiplicative weight applied to the inherited distillation loss. Defaults to ``1.0``.
        expert (nn.Module | None):
            The expert itself instead of a path to it: an ``ExpertPolicy``, or any callable module with an optional
            ``reset(done)``.  Exactly one of ``expert_path`` and ``expert`` is given.
    """

    def __init__(self, expert_path: str = "", observation_name: str = "observation", weight: float = 1.0, *,
                 expert: nn.Module | None = None):
        super().__init__(weight=weight)
        self.expert_path = expert_path
        self.observation_name = observation_name
        self._given_expert = expert

        # Runtime attributes
        self.expert: nn.Module

    def init(self):
        from cusrl_amd.nn.expert import ExpertPolicy

        super().init()
        if bool(self.expert_path) == (self._given_expert is not None):
            raise ValueError("'expert_path' cannot be empty")
        device = self.agent.device
        if self._given_expert is not None:
            expert = self._given_expert
            if isinstance(expert, nn.Module) and not isinstance(expert, torch.jit.ScriptModule):
                expert = expert.to(device)
        else:
            # (a file of another format is never unpickled: it is TorchScript, the reference's contract, or an error)
            expert = ExpertPolicy.try_load(self.expert_path, map_location=device)
            if expert is None:
                from cusrl_amd.nn.deployed import DeployedPolicy

                # a policy file written by ActorCritic.export: callable, with a reset(done) — all this hook needs
                expert = DeployedPolicy.try_load(self.expert_path, map_location=device)
            if expert is None:
                expert = torch.jit.load(self.expert_path, map_location=device)
        # a plain attribute: not registered with the agent, so neither checkpointed nor handed to an optimizer
        self.expert = expert

    @property
    def native_expert(self) -> bool:
        from cusrl_amd.nn.expert import ExpertPolicy

        return isinstance(getattr(self, "expert", None), ExpertPolicy)

    # A native expert's query is shape-static device work that reads the observation and writes a leaf of its own, so it may
    # be captured and the step epilogue may fuse with the buffer append; anything else (TorchScript, a user's module) may keep
    # state or read back to the host: the rollout then stays host-driven (template/graphs.py GraphedRolloutStep.supported).
    @property
    def rollout_capture_safe(self) -> bool:
        return self.native_expert

    @property
    def post_step_device_free(self) -> bool:
        return self.native_expert

    def eager_phases(self) -> tuple[str, ...]:
        return () if self.native_expert else ("step",)

    @torch.no_grad()
    def post_step(self, transition):
        transition[self.target_name] = self.expert(transition[self.observation_name])
        if hasattr(self.expert, "reset"):
            self.expert.reset(transition["done"].squeeze(-1))
