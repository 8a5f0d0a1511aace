from cusrl_amd.template.actor_critic import ActorCritic, ActorCriticFactory
from cusrl_amd.template.agent import Agent, AgentFactory
from cusrl_amd.template.buffer import Buffer, Sampler
from cusrl_amd.template.environment import Environment, EnvironmentSpec
from cusrl_amd.template.hook import Hook, HookComposite
from cusrl_amd.template.logger import Logger, LoggerFactory, LoggerFactoryLike, make_logger_factory
from cusrl_amd.template.optimizer import OptimizerCollection, OptimizerFactory, build_optimizer
from cusrl_amd.template.player import Player, PlayerHook, PlayerHookComposite
from cusrl_amd.template.trainer import Trainer, TrainerHook
from cusrl_amd.template.trial import Trial

__all__ = [
    "ActorCritic",
    "ActorCriticFactory",
    "Agent",
    "AgentFactory",
    "Buffer",
    "Environment",
    "EnvironmentSpec",
    "Hook",
    "HookComposite",
    "Logger",
    "LoggerFactory",
    "LoggerFactoryLike",
    "OptimizerCollection",
    "OptimizerFactory",
    "Player",
    "PlayerHook",
    "PlayerHookComposite",
    "Sampler",
    "Trainer",
    "TrainerHook",
    "Trial",
    "build_optimizer",
    "make_logger_factory",
]
