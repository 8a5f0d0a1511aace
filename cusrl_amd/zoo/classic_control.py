"""The five classic-control ``ppo`` experiments with the hyper-parameters, env counts, iteration counts and checkpoint intervals
of the reference's registrations (cusrl/zoo/gym/classic_control.py:7-142), each on this package's device-resident environment
(``cusrl_amd.environment``) instead of a gymnasium vector env."""

from functools import partial

from cusrl_amd.environment import make
from cusrl_amd.preset import PpoAgentFactory
from cusrl_amd.zoo import register_experiment

__all__: list[str] = []

_NETWORK = dict(actor_hidden_dims=(64, 64), critic_hidden_dims=(64, 64), activation_fn="Tanh")


def _register(environment_name: str, num_envs: int, num_iterations: int, checkpoint_interval: int, **agent_kwargs):
    register_experiment(environment_name, "ppo", PpoAgentFactory, {**_NETWORK, **agent_kwargs}, partial(make, environment_name),
                        {"num_envs": num_envs}, num_iterations, checkpoint_interval)


_register("Acrobot-v1", 16, 500, 50, num_steps_per_update=16, action_space_type="discrete", lr=3e-4, sampler_epochs=4,
          sampler_mini_batches=64, orthogonal_init=False, normalize_observation=True, gae_gamma=0.99, gae_lamda=0.94,
          entropy_loss_weight=0.0, max_grad_norm=0.5)
_register("CartPole-v1", 8, 400, 50, num_steps_per_update=32, action_space_type="discrete", lr=1e-3, sampler_epochs=20,
          sampler_mini_batches=1, gae_gamma=0.8, gae_lamda=0.98, entropy_loss_weight=0.0, max_grad_norm=0.5)
_register("MountainCar-v0", 16, 2000, 500, num_steps_per_update=16, action_space_type="discrete", lr=3e-4, sampler_epochs=4,
          sampler_mini_batches=4, orthogonal_init=False, normalize_observation=True, gae_gamma=0.99, gae_lamda=0.98,
          entropy_loss_weight=0.0, max_grad_norm=0.5)
_register("MountainCarContinuous-v0", 1, 2500, 500, num_steps_per_update=8, value_loss_weight=0.19, lr=7.77e-5, sampler_epochs=10,
          sampler_mini_batches=1, orthogonal_init=False, init_distribution_std=0.04, normalize_observation=True, gae_gamma=0.9999,
          gae_lamda=0.9, surrogate_clip_ratio=0.1, entropy_loss_weight=0.00429, max_grad_norm=5.0)
_register("Pendulum-v1", 4, 50, 25, num_steps_per_update=1024, sampler_epochs=10, sampler_mini_batches=64, normalize_observation=True,
          gae_gamma=0.9, lr=1e-3, entropy_loss_weight=0.0, max_grad_norm=0.5)
