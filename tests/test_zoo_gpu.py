"""The experiment zoo on the GPU: every registered spec's training loop, and the ``train`` command, where the agent's update path
exists.  Registry, values and the command line's host side: tests/test_zoo.py."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("Acrobot-v1", "CartPole-v1", "MountainCar-v0", "MountainCarContinuous-v0", "Pendulum-v1")


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


@pytest.mark.parametrize("name", NAMES)
def test_make_trainer_runs_its_loop(cusrl, name):
    """``make_trainer(num_envs=4, num_iterations=2)`` of each of the five on its device-resident env: two rollouts and two updates
    with the registered hyper-parameters, finite parameters and an env that has moved."""
    spec = cusrl.zoo.get_experiment(name, "ppo")
    cusrl.set_global_seed(4)
    trainer = spec.make_trainer(num_envs=4, num_iterations=2, device=DEV)
    env = trainer.environment
    assert env.num_instances == 4 and env.capturable and env.state.is_cuda
    trainer.run_training_loop()
    assert trainer.iteration == 2 and trainer.stats.total_steps == 2 * 4 * spec.agent_factory_kwargs["num_steps_per_update"]
    assert all(torch.isfinite(p).all() for p in trainer.agent.parameters())
    assert (env.episode >= 1).all() and torch.isfinite(env.state).all()


def test_the_train_command_leaves_a_checkpoint(cusrl, tmp_path):
    from cusrl_amd.__main__ import main

    assert main(["train", "--environment", "CartPole-v1", "--algorithm", "ppo", "--num-iterations", "1", "--num-envs", "4", "--device", DEV,
                 "--log-dir", str(tmp_path)]) == 0
    names = sorted(path.name for path in tmp_path.glob("*_CartPole-v1_ppo/ckpt/ckpt_*.pt"))
    assert names == ["ckpt_0.pt", "ckpt_1.pt"]
    checkpoint = torch.load(next(tmp_path.glob("*_CartPole-v1_ppo/ckpt/ckpt_1.pt")), weights_only=False)
    assert checkpoint["iteration"] == 1 and tuple(checkpoint["environment"]["state"].shape) == (4, 4)
