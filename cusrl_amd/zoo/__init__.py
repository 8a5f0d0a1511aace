"""The experiment registry (counterpart of cusrl/zoo/registry.py and the ``zoo/gym`` registrations): a named pairing of an
environment factory, an agent factory and the length of a training run, so that "PPO on CartPole as the reference configures it" is
``zoo.get_experiment("CartPole-v1", "ppo").make_trainer()`` or ``python -m cusrl_amd train --environment CartPole-v1 --algorithm
ppo``.  Host-only: nothing here launches a kernel; what a trainer built here runs is the package's usual device path."""

from __future__ import annotations

from collections.abc import Callable, Mapping
from dataclasses import dataclass, field
from typing import Any

from cusrl_amd.template.agent import AgentFactory
from cusrl_amd.template.environment import Environment
from cusrl_amd.template.trainer import Trainer

__all__ = ["ExperimentSpec", "get_experiment", "list_experiments", "register_experiment"]


@dataclass(frozen=True)
class ExperimentSpec:
    environment_name: str
    algorithm_name: str
    agent_factory_cls: Callable[..., AgentFactory]
    agent_factory_kwargs: Mapping[str, Any]
    environment_factory: Callable[..., Environment]
    environment_factory_kwargs: Mapping[str, Any] = field(default_factory=dict)
    """Holds ``num_envs``; everything else goes to ``environment_factory`` as it is."""
    num_iterations: int = 1000
    checkpoint_interval: int = 50

    @property
    def name(self) -> str:
        return f"{self.environment_name}_{self.algorithm_name}"

    @property
    def num_envs(self) -> int:
        return int(self.environment_factory_kwargs.get("num_envs", 1))

    def make_agent_factory(self, device=None, **agent_overrides) -> AgentFactory:
        return self.agent_factory_cls(**{**self.agent_factory_kwargs, **agent_overrides, "device": device})

    def make_environment(self, num_envs: int | None = None, device=None, seed: int | None = None) -> Environment:
        kwargs = {key: value for key, value in self.environment_factory_kwargs.items() if key != "num_envs"}
        return self.environment_factory(self.num_envs if num_envs is None else int(num_envs), device=device, seed=seed, **kwargs)

    def make_trainer(self, num_envs: int | None = None, num_iterations: int | None = None, device=None, seed: int | None = None,
                     **agent_overrides) -> Trainer:
        """A :class:`Trainer` of this experiment.  ``agent_overrides`` replace fields of the agent factory; ``logger_factory``,
        ``checkpoint_path`` and ``verbose`` among them go to the trainer instead."""
        trainer_kwargs = {key: agent_overrides.pop(key) for key in ("logger_factory", "checkpoint_path", "verbose")
                          if key in agent_overrides}
        trainer_kwargs.setdefault("verbose", False)
        return Trainer(self.make_environment(num_envs, device, seed), self.make_agent_factory(device, **agent_overrides),
                       num_iterations=self.num_iterations if num_iterations is None else int(num_iterations),
                       checkpoint_interval=self.checkpoint_interval, **trainer_kwargs)


_REGISTRY: dict[str, ExperimentSpec] = {}


def register_experiment(environment_name: str, algorithm_name: str, agent_factory_cls, agent_factory_kwargs: Mapping[str, Any],
                        environment_factory, environment_factory_kwargs: Mapping[str, Any] | None = None, num_iterations: int = 1000,
                        checkpoint_interval: int = 50) -> ExperimentSpec:
    spec = ExperimentSpec(environment_name, algorithm_name, agent_factory_cls, dict(agent_factory_kwargs), environment_factory,
                          dict(environment_factory_kwargs or {}), int(num_iterations), int(checkpoint_interval))
    if spec.name in _REGISTRY:
        raise ValueError(f"experiment {spec.name!r} is already registered")
    _REGISTRY[spec.name] = spec
    return spec


def get_experiment(environment_name: str, algorithm_name: str) -> ExperimentSpec:
    name = f"{environment_name}_{algorithm_name}"
    if name not in _REGISTRY:
        raise ValueError(f"unknown experiment {name!r}; registered: {', '.join(list_experiments()) or 'none'}")
    return _REGISTRY[name]


def list_experiments() -> list[str]:
    return sorted(_REGISTRY)


from cusrl_amd.zoo import classic_control  # noqa: E402, F401  (registers the five classic-control experiments)
