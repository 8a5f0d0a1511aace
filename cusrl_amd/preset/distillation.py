"""The `distillation` preset (counterpart of cusrl/preset/distillation.py:18-92): a student actor trained on the actions of a
frozen expert.  Same hook order, field names and defaults as the reference; the factory additionally takes the expert as a
module (``expert``), which is how a native ``nn.ExpertPolicy`` built by ``ExpertPolicy.from_actor`` gets in without a file.

The critic is a ``Value`` on a ``StubModule``: it exists because an ``ActorCritic`` has one, it is never evaluated, and its head
receives no gradient (the optimizer leaves such parameters alone)."""

from __future__ import annotations

from collections.abc import Sequence
from dataclasses import dataclass

import torch

from cusrl_amd import hook as hooks
from cusrl_amd.nn import Actor, Mlp, NormalDist, StubModule, Value
from cusrl_amd.preset.ppo import AdamFactory
from cusrl_amd.sampler import AutoMiniBatchSampler
from cusrl_amd.template.actor_critic import ActorCritic, ActorCriticFactory
from cusrl_amd.template.agent import AgentFactory
from cusrl_amd.template.environment import EnvironmentSpec
from cusrl_amd.template.hook import Hook

__all__ = ["DistillationAgentFactory", "distillation_hook_suite"]


def distillation_hook_suite(
    expert_path: str = "",
    expert_observation_name: str = "observation",
    normalize_observation: bool = False,
    max_grad_norm: float | None = 1.0,
    *,
    expert: torch.nn.Module | None = None,
) -> list[Hook]:
    suite = [
        hooks.ObservationNormalization() if normalize_observation else None,
        hooks.OnPolicyPreparation(),
        hooks.PolicyDistillation(expert_path, expert_observation_name, expert=expert),
        hooks.GradientClipping(max_grad_norm),
    ]
    return [h for h in suite if h is not None]


@dataclass(kw_only=True)
class DistillationAgentFactory(AgentFactory):
    num_steps_per_update: int = 24
    actor_hidden_dims: Sequence[int] = (256, 128)
    activation_fn: str | type[torch.nn.Module] = "ReLU"
    lr: float = 2e-4
    sampler_epochs: int = 1
    sampler_mini_batches: int = 8
    init_distribution_std: float | None = None
    expert_path: str = ""
    """Path to the expert: a file written by ``ExpertPolicy.save`` or a TorchScript module that maps observations to actions."""
    expert_observation_name: str = "observation"
    normalize_observation: bool = False
    max_grad_norm: float | None = 1.0
    expert: torch.nn.Module | None = None
    """The expert itself instead of ``expert_path`` (extension): an ``ExpertPolicy`` or any callable module."""

    def to_underlying(self) -> ActorCriticFactory:
        return ActorCriticFactory(
            num_steps_per_update=self.num_steps_per_update,
            actor_factory=Actor.Factory(
                backbone_factory=Mlp.Factory(hidden_dims=self.actor_hidden_dims, activation_fn=self.activation_fn,
                                             ends_with_activation=True),
                distribution_factory=NormalDist.Factory(init_std=self.init_distribution_std),
            ),
            critic_factory=Value.Factory(backbone_factory=StubModule.Factory()),
            optimizer_factory=AdamFactory(defaults={"lr": self.lr, **({"capturable": True, "fused": True} if self.compile else {})}),
            sampler=AutoMiniBatchSampler(num_epochs=self.sampler_epochs, num_mini_batches=self.sampler_mini_batches),
            hooks=distillation_hook_suite(
                expert_path=self.expert_path,
                expert_observation_name=self.expert_observation_name,
                normalize_observation=self.normalize_observation,
                max_grad_norm=self.max_grad_norm,
                expert=self.expert,
            ),
            name=self.name,
            device=self.device,
            compile=self.compile,
            autocast=self.autocast,
        )

    def __call__(self, environment_spec: EnvironmentSpec) -> ActorCritic:
        return self.to_underlying()(environment_spec)
