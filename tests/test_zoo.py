"""The experiment registry ``cusrl_amd.zoo`` and its command line ``python -m cusrl_amd`` (no GPU): the five classic-control
``ppo`` registrations against the reference's values (cusrl/zoo/gym/classic_control.py:7-142, copied into ``EXPECTED`` below), the
registry's errors, the trainers the specs build, and the command line in-process.

The issue behind this file asks that every spec's training loop run here for two iterations on CPU envs.  The environments have a
host form and that part runs below (reset, act, step through the trainer's own objects); the agent's update path does not — buffer
append, GAE and the PPO step exist as HIP kernels only, by design (``ops.require_device``) — so what is asserted on
the CPU is that the loop REFUSES there instead of quietly computing something else, and the two-iteration loops of all five specs
and the one-iteration ``train`` command run where they can: tests/test_zoo_gpu.py."""

import pytest
import torch

NETWORK = dict(actor_hidden_dims=(64, 64), critic_hidden_dims=(64, 64), activation_fn="Tanh")
EXPECTED = {  # name: (env class, num_envs, num_iterations, checkpoint_interval, agent kwargs)
    "Acrobot-v1": ("Acrobot", 16, 500, 50, dict(
        num_steps_per_update=16, action_space_type="discrete", lr=3e-4, sampler_epochs=4, sampler_mini_batches=64,
        orthogonal_init=False, normalize_observation=True, gae_gamma=0.99, gae_lamda=0.94, entropy_loss_weight=0.0,
        max_grad_norm=0.5)),
    "CartPole-v1": ("CartPole", 8, 400, 50, dict(
        num_steps_per_update=32, action_space_type="discrete", lr=1e-3, sampler_epochs=20, sampler_mini_batches=1, gae_gamma=0.8,
        gae_lamda=0.98, entropy_loss_weight=0.0, max_grad_norm=0.5)),
    "MountainCar-v0": ("MountainCar", 16, 2000, 500, dict(
        num_steps_per_update=16, action_space_type="discrete", lr=3e-4, sampler_epochs=4, sampler_mini_batches=4,
        orthogonal_init=False, normalize_observation=True, gae_gamma=0.99, gae_lamda=0.98, entropy_loss_weight=0.0,
        max_grad_norm=0.5)),
    "MountainCarContinuous-v0": ("MountainCarContinuous", 1, 2500, 500, dict(
        num_steps_per_update=8, value_loss_weight=0.19, lr=7.77e-5, sampler_epochs=10, sampler_mini_batches=1, orthogonal_init=False,
        init_distribution_std=0.04, normalize_observation=True, gae_gamma=0.9999, gae_lamda=0.9, surrogate_clip_ratio=0.1,
        entropy_loss_weight=0.00429, max_grad_norm=5.0)),
    "Pendulum-v1": ("Pendulum", 4, 50, 25, dict(
        num_steps_per_update=1024, sampler_epochs=10, sampler_mini_batches=64, normalize_observation=True, gae_gamma=0.9, lr=1e-3,
        entropy_loss_weight=0.0, max_grad_norm=0.5)),
}


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def test_the_registry_lists_exactly_the_five(cusrl):
    assert cusrl.zoo.list_experiments() == sorted(f"{name}_ppo" for name in EXPECTED)


def test_double_registration_and_unknown_keys_raise(cusrl):
    zoo = cusrl.zoo
    spec = zoo.get_experiment("CartPole-v1", "ppo")
    with pytest.raises(ValueError, match="already registered"):
        zoo.register_experiment("CartPole-v1", "ppo", spec.agent_factory_cls, spec.agent_factory_kwargs, spec.environment_factory,
                                spec.environment_factory_kwargs, spec.num_iterations, spec.checkpoint_interval)
    assert zoo.get_experiment("CartPole-v1", "ppo") is spec and len(zoo.list_experiments()) == 5
    for key in (("CartPole-v1", "sac"), ("CartPole", "ppo"), ("Acrobot", "ppo")):
        with pytest.raises(ValueError, match="Acrobot-v1_ppo, CartPole-v1_ppo, MountainCar-v0_ppo"):
            zoo.get_experiment(*key)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_registration_holds_the_reference_values(cusrl, name):
    cls, num_envs, num_iterations, checkpoint_interval, agent_kwargs = EXPECTED[name]
    spec = cusrl.zoo.get_experiment(name, "ppo")
    assert (spec.environment_name, spec.algorithm_name, spec.name) == (name, "ppo", f"{name}_ppo")
    assert spec.agent_factory_cls is cusrl.preset.PpoAgentFactory
    assert dict(spec.agent_factory_kwargs) == {**NETWORK, **agent_kwargs}
    assert (spec.num_envs, spec.num_iterations, spec.checkpoint_interval) == (num_envs, num_iterations, checkpoint_interval)
    factory = spec.make_agent_factory(device="cpu", lr=1.0)  # an override replaces a field, the rest stays
    assert factory.lr == 1.0 and factory.gae_gamma == agent_kwargs["gae_gamma"] and factory.device == "cpu"
    env = spec.make_environment(device="cpu", seed=1)
    assert type(env) is getattr(cusrl.environment, cls) and env.num_instances == num_envs


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_make_trainer_on_the_cpu(cusrl, name):
    """``make_trainer(num_envs=4, num_iterations=2, device="cpu")``: the trainer, its env in host form and its agent are built as
    registered; the host-form part of an env step runs (reset with randomised progress, ``act``, ``step``); the loop itself is
    refused on CPU tensors — the agent's update path has no host form — and runs in tests/test_zoo_gpu.py."""
    cls, _, _, checkpoint_interval, agent_kwargs = EXPECTED[name]
    spec = cusrl.zoo.get_experiment(name, "ppo")
    trainer = spec.make_trainer(num_envs=4, num_iterations=2, device="cpu", seed=3)
    assert isinstance(trainer, cusrl.Trainer) and type(trainer.environment) is getattr(cusrl.environment, cls)
    assert trainer.environment.num_instances == 4 and trainer.environment.device.type == "cpu"
    assert (trainer.num_iterations, trainer.checkpoint_interval, trainer.iteration) == (2, checkpoint_interval, 0)
    agent = trainer.agent
    assert agent.device.type == "cpu" and agent.num_steps_per_update == agent_kwargs["num_steps_per_update"]
    observation, state, _ = trainer.environment.reset(randomize_episode_progress=True)
    action = agent.act(observation, state)
    assert action.shape == (4, trainer.environment.action_dim)
    next_observation, _, reward, terminated, truncated, _ = trainer.environment.step(action)
    assert next_observation.shape == observation.shape and reward.shape == terminated.shape == truncated.shape == (4, 1)
    assert torch.isfinite(next_observation).all()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spec.make_trainer(num_envs=4, num_iterations=2, device="cpu", seed=3).run_training_loop()
    assert spec.make_trainer(device="cpu").num_iterations == spec.num_iterations  # (the defaults are the registration's)


def test_the_command_line_lists_the_five(cusrl, capsys):
    from cusrl_amd.__main__ import main

    assert main(["list-experiments"]) == 0
    assert capsys.readouterr().out.split() == sorted(f"{name}_ppo" for name in EXPECTED)
    with pytest.raises(SystemExit):
        main(["play"])  # (no play, export or benchmark subcommands)
    with pytest.raises(ValueError, match="unknown experiment"):
        main(["train", "--environment", "Acrobot", "--algorithm", "ppo", "--device", "cpu"])


def test_the_train_command_builds_the_run_and_leaves_a_checkpoint(cusrl, tmp_path):
    """On the CPU the command goes as far as a process without a GPU can: the run directory, the checkpoint the trainer writes
    before its loop, the env reset in host form; with zero iterations it returns 0.  One iteration is refused like any update on CPU
    tensors (it runs in tests/test_zoo_gpu.py)."""
    from cusrl_amd.__main__ import main

    arguments = ["train", "--environment", "CartPole-v1", "--algorithm", "ppo", "--num-envs", "4", "--device", "cpu", "--seed", "1",
                 "--log-dir", str(tmp_path)]
    assert main([*arguments, "--num-iterations", "0"]) == 0
    checkpoints = sorted(tmp_path.glob("*_CartPole-v1_ppo/ckpt/ckpt_*.pt"))
    assert [path.name for path in checkpoints] == ["ckpt_0.pt"]
    checkpoint = torch.load(checkpoints[0], weights_only=False)
    assert checkpoint["iteration"] == 0 and checkpoint["environment"]["task"] == "CartPole"
    assert tuple(checkpoint["environment"]["state"].shape) == (4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        main([*arguments, "--num-iterations", "1"])
