"""``cusrl_play_epilogue`` against its numpy restatement, bit for bit, and the play loop end to end on the device (GPU).

Kernel cases (tests/_player.py): N in {1, B - 1, B, B + 1, 2 B + 1, 16 B + 1} for the block size B read from csrc/common.hpp, D in
{1, 3}, five done patterns, targets {1, 3}; six consecutive launches on ONE workspace zeroed once, parity alternating — the case
that fails when the self-reset or the ticket is wrong — with ``unfinished_out`` once a device word and once pinned host memory.
Rewards are fp32 integers in {-2..2}: every sum is exact in any order, so every assertion is ``torch.equal``.  Every buffer is
sized exactly and sits between 64 poisoned elements on either side."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _player
from _player import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = 6


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


class DeviceState:
    """The launch-to-launch buffers of one case, each exactly sized between guard bands."""

    def __init__(self, N, D, R, pinned_unfinished: bool):
        z = lambda shape, dtype: Guarded(np.zeros(shape), dtype, DEV)  # noqa: E731
        self.episode_rew, self.episode_len = z((N, D), torch.float32), z((N,), torch.float32)
        self.ring_rew, self.ring_len = z((R, D), torch.float32), z((R,), torch.float32)
        self.counter, self.step_reward_sum = z((2,), torch.int64), z((D,), torch.float64)
        self.indices, self.count = z((N,), torch.int64), z((1,), torch.int32)
        self.done = z((N, 1), torch.bool)
        self.episode_count, self.workspace = z((N,), torch.int64), z((2,), torch.int32)
        self.unfinished_guard = None if pinned_unfinished else z((1,), torch.int32)
        self.unfinished = torch.zeros(1, dtype=torch.int32).pin_memory() if pinned_unfinished else self.unfinished_guard.tensor
        self.guards = [v for v in vars(self).values() if isinstance(v, Guarded)]

    def carried(self):
        return (self.episode_rew, self.episode_len, self.ring_rew, self.ring_len, self.counter, self.step_reward_sum)


def launch_inputs(N, D, pattern, launch):
    terminated, truncated = _player.done_pattern(pattern, N, launch)
    reward = _player.lattice((N, D), seed=31 * N + 7 * D + launch)
    return reward, terminated, truncated


def assert_state(device: DeviceState, state: _player.EpilogueState, what):
    expected = (state.episode_rew, state.episode_len, state.ring_rew, state.ring_len, state.counter, state.step_reward_sum)
    for name, got, want in zip(("episode_rew", "episode_len", "ring_rew", "ring_len", "num_episodes", "step_reward_sum"),
                               device.carried(), expected):
        assert torch.equal(got.tensor.cpu(), torch.from_numpy(np.ascontiguousarray(want))), (name, what)


@pytest.mark.parametrize("pattern", _player.PATTERNS)
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("N", _player.kernel_sizes())
def test_kernel_matches_the_restatement_over_six_launches(cusrl, N, D, pattern):
    from cusrl_amd import ops

    for target in (1, 3):
        for pinned in (False, True):
            device, state = DeviceState(N, D, N, pinned), _player.EpilogueState(N, D, N)
            for launch in range(LAUNCHES):
                what = (target, pinned, launch)
                parity = launch % 2
                reward, terminated, truncated = launch_inputs(N, D, pattern, launch)
                inputs = (Guarded(reward, torch.float32, DEV), Guarded(terminated[:, None], torch.bool, DEV),
                          Guarded(truncated[:, None], torch.bool, DEV))
                device.count.tensor.fill_(-1)
                device.unfinished.fill_(-1)
                ops.play_epilogue(inputs[0].tensor, inputs[1].tensor, inputs[2].tensor, device.done.tensor, device.episode_rew.tensor,
                                  device.episode_len.tensor, device.ring_rew.tensor, device.ring_len.tensor, device.counter.tensor,
                                  device.step_reward_sum.tensor, device.indices.tensor, device.count.tensor, parity,
                                  device.episode_count.tensor, target, device.unfinished, device.workspace.tensor)
                torch.cuda.synchronize()
                done, indices, unfinished = _player.play_epilogue_restated(state, reward, terminated, truncated, parity, target)
                assert torch.equal(device.episode_count.tensor.cpu(), torch.from_numpy(state.episode_count)), what
                assert int(device.unfinished[0]) == unfinished, what
                assert int(device.count.tensor[0]) == indices.size, what
                assert torch.equal(device.indices.tensor[: indices.size].cpu(), torch.from_numpy(indices)), what
                assert torch.equal(device.done.tensor.cpu().reshape(-1), torch.from_numpy(done)), what
                assert_state(device, state, what)
                assert not device.workspace.tensor.any(), ("the workspace must read zero after every launch", what)
                assert all(g.intact() for g in device.guards) and all(g.intact() for g in inputs), ("guard band overwritten", what)


@pytest.mark.parametrize("N", _player.kernel_sizes())
def test_parity_with_the_step_epilogue(cusrl, N):
    """The same inputs through ``cusrl_step_epilogue`` and ``cusrl_play_epilogue``: everything the two share is identical."""
    from cusrl_amd import ops

    D = 3
    step, play = DeviceState(N, D, N, False), DeviceState(N, D, N, False)
    for launch in range(3):
        parity = launch % 2
        reward, terminated, truncated = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in launch_inputs(N, D, "bernoulli", launch))
        terminated, truncated = terminated[:, None].contiguous(), truncated[:, None].contiguous()
        for device in (step, play):
            device.count.tensor.fill_(-1)
        ops.step_epilogue(reward, terminated, truncated, step.done.tensor, step.episode_rew.tensor, step.episode_len.tensor,
                          step.ring_rew.tensor, step.ring_len.tensor, step.counter.tensor, step.step_reward_sum.tensor,
                          step.indices.tensor, step.count.tensor, parity)
        ops.play_epilogue(reward, terminated, truncated, play.done.tensor, play.episode_rew.tensor, play.episode_len.tensor,
                          play.ring_rew.tensor, play.ring_len.tensor, play.counter.tensor, play.step_reward_sum.tensor,
                          play.indices.tensor, play.count.tensor, parity, play.episode_count.tensor, 2, play.unfinished,
                          play.workspace.tensor)
        torch.cuda.synchronize()
        count = int(step.count.tensor[0])
        assert count == int(play.count.tensor[0]) == int((terminated | truncated).sum())
        assert torch.equal(step.indices.tensor[:count], play.indices.tensor[:count]) and torch.equal(step.done.tensor, play.done.tensor)
        for a, b in zip(step.carried(), play.carried()):
            assert torch.equal(a.tensor, b.tensor)
        assert all(g.intact() for g in step.guards + play.guards)


def test_error_codes_launch_nothing(cusrl):
    from cusrl_amd import _native

    before = dict(_native.launch_counts)
    _player.check_error_codes(_native.lib())  # host-side checks of the raw entry: the pointers are never dereferenced
    assert _native.launch_counts == before
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
N_ENVS, OBS, ACT = 64, 8, 3


def build(cusrl, seed=3, capturable=True, normalize=False, **limits):
    """Seeded env + freshly built agent: about one finished episode per env every 8 steps."""
    cusrl.set_global_seed(seed)

    class Environment(cusrl.testing.SyntheticEnvironment):
        def __init__(self):
            super().__init__(N_ENVS, OBS, ACT, terminate_prob=0.08, truncate_prob=0.05, device=DEV, seed=seed)
            if not capturable:
                self.capturable = self.generator_free = False

    environment = Environment()
    factory = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(32, 16), critic_hidden_dims=(32, 16), num_steps_per_update=8,
                                           sampler_epochs=1, sampler_mini_batches=2, normalize_observation=normalize, device=DEV)
    return environment, factory


def play(cusrl, tmp_path, tag, hooks=(), **kwargs):
    build_kwargs = {k: kwargs.pop(k) for k in ("seed", "capturable") if k in kwargs}
    environment, factory = build(cusrl, **build_kwargs)
    saver = cusrl.hook.SaveTransition(tmp_path / tag)
    player = cusrl.Player(environment, factory, hooks=[saver, *hooks], progress_bar=False, **kwargs)
    metrics = player.run_playing_loop()
    with np.load(tmp_path / f"{tag}.npz") as saved:
        arrays = {key: saved[key] for key in saved.files}
    return player, metrics, arrays


def test_num_episodes_ends_where_the_saved_flags_say(cusrl, tmp_path):
    player, metrics, saved = play(cusrl, tmp_path, "two", num_episodes=2)
    assert player.device_bookkeeping is True and player.episode_count.is_cuda and player.episode_count.dtype == torch.int64
    assert saved["observation"].shape[1:] == (N_ENVS, OBS) and saved["action"].shape[1:] == (N_ENVS, ACT)
    assert saved["terminated"].dtype == bool and saved["terminated"].shape[1:] == (N_ENVS, 1) and saved["reward"].dtype == np.float32
    done = (saved["terminated"] | saved["truncated"])[..., 0]
    steps, counts, expected, bounds = _player.recompute_play(saved["reward"], done, 2, N_ENVS)
    assert player.step_count == steps == done.shape[0]  # the loop stopped at the first step every env had its two episodes
    assert torch.equal(player.episode_count.cpu(), torch.from_numpy(counts))
    for name in expected:
        error = np.abs(np.asarray(metrics[name], np.float64) - expected[name])
        print(f"{name}: error {np.max(error):.3e}, {np.max(error / np.maximum(bounds[name], 1e-300)):.3f} of the bound")
        assert np.all(error <= bounds[name]), (name, error, bounds[name])


def test_device_and_host_bookkeeping_agree(cusrl, tmp_path):
    runs = {"device": dict(device_bookkeeping=True), "host": dict(device_bookkeeping=False),
            "count_out": dict(device_bookkeeping=True, capturable=False)}
    results = {tag: play(cusrl, tmp_path, tag, num_episodes=2, **kwargs) for tag, kwargs in runs.items()}
    assert [results[tag][0].device_bookkeeping for tag in runs] == [True, False, True]
    reference, _, saved = results["host"]
    assert not reference.episode_count.is_cuda
    for tag in ("device", "count_out"):
        player, _, other = results[tag]
        assert player.step_count == reference.step_count and torch.equal(player.episode_count.cpu(), reference.episode_count)
        for key in ("terminated", "truncated", "reward"):
            assert np.array_equal(other[key], saved[key]), (tag, key)


def test_deterministic_actions_are_the_actors_mean(cusrl, tmp_path):
    player, _, saved = play(cusrl, tmp_path, "det", num_steps=6)
    assert player.agent.inference_mode and player.agent.deterministic
    environment, factory = build(cusrl)  # same seed: the same initial parameters
    agent = factory.from_environment(environment)
    for t in (0, 2, 5):
        observation = torch.from_numpy(saved["observation"][t]).to(DEV)
        with torch.no_grad():
            action, _ = agent.actor.act(observation, deterministic=True)
        assert torch.equal(action.cpu(), torch.from_numpy(saved["action"][t])), t


def test_host_reads_per_step(cusrl, monkeypatch):
    """Capturable env, no hooks: with ``num_steps`` only the loop reads nothing back; with ``num_episodes`` exactly one pinned word
    per step."""
    from cusrl_amd import ops

    reads = {"wait": 0, "item": 0, "tolist": 0}
    at_report = {}

    def counted(name, original):
        def wrapper(*args, **kwargs):
            reads[name] += 1
            return original(*args, **kwargs)

        return wrapper

    monkeypatch.setattr(ops.HostCounter, "wait", counted("wait", ops.HostCounter.wait))
    monkeypatch.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "tolist", counted("tolist", torch.Tensor.tolist))
    report = cusrl.Player._get_metrics_report

    def report_marks_the_end_of_the_loop(self):
        at_report.update(reads)
        return report(self)

    monkeypatch.setattr(cusrl.Player, "_get_metrics_report", report_marks_the_end_of_the_loop)
    environment, factory = build(cusrl)
    player = cusrl.Player(environment, factory, num_steps=16, progress_bar=False)
    for key in reads:
        reads[key] = 0
    player.run_playing_loop()
    assert player.step_count == 16 and player.device_bookkeeping is True
    assert at_report == {"wait": 0, "item": 0, "tolist": 0}

    environment, factory = build(cusrl)
    player = cusrl.Player(environment, factory, num_episodes=1, progress_bar=False)
    for key in reads:
        reads[key] = 0
    player.run_playing_loop()
    assert at_report == {"wait": player.step_count, "item": 0, "tolist": 0} and player.step_count > 1


def test_reset_hook_receives_ascending_device_indices(cusrl, tmp_path):
    received = []

    class Resets(cusrl.PlayerHook):
        def reset(self, indices):
            assert isinstance(indices, torch.Tensor) and indices.is_cuda and indices.dtype == torch.int64 and indices.numel() > 0
            received.append((self.player.step_count - 1, indices))

    player, _, saved = play(cusrl, tmp_path, "resets", hooks=[Resets()], num_steps=12)
    done = (saved["terminated"] | saved["truncated"])[..., 0]
    steps = np.concatenate([np.full(indices.numel(), step) for step, indices in received])
    envs = torch.cat([indices for _, indices in received]).cpu().numpy()
    expected_steps, expected_envs = np.nonzero(done)  # row-major: by step, ascending env within a step
    assert np.array_equal(steps, expected_steps) and np.array_equal(envs, expected_envs)


def test_train_then_play_round_trip(cusrl, tmp_path):
    environment, factory = build(cusrl, normalize=True)
    logger_factory = cusrl.Logger.Factory(tmp_path, name="run", add_datetime_prefix=False)
    # (the trainer's checkpoint cadence argument is `checkpoint_interval`)
    trainer = cusrl.Trainer(environment, factory, logger_factory=logger_factory, num_iterations=2, checkpoint_interval=1, verbose=False)
    trainer.run_training_loop()
    assert sorted(p.name for p in (tmp_path / "run" / "ckpt").iterdir()) == ["ckpt_0.pt", "ckpt_1.pt", "ckpt_2.pt"]

    environment, factory = build(cusrl, seed=11, normalize=True)  # other initial parameters: equality below comes from the file
    player = cusrl.Player(environment, factory, checkpoint_path=str(tmp_path), num_steps=4, progress_bar=False)
    assert player.trial.iteration == 2 and player.trial.home == (tmp_path / "run").resolve()
    trained, loaded = dict(trainer.agent.named_parameters()), dict(player.agent.named_parameters())
    assert trained.keys() == loaded.keys() and len(trained) > 0
    for name in trained:
        assert torch.equal(trained[name], loaded[name]), name
    from cusrl_amd.nn.rms import RunningMeanStd

    def rms_buffers(agent):
        found = {}
        for hook in agent.hook:
            for module_name, module in hook._modules.items():
                if isinstance(module, RunningMeanStd):
                    found.update({f"{module_name}.{key}": value for key, value in module.state_dict().items()})
        return found

    trained_rms, loaded_rms = rms_buffers(trainer.agent), rms_buffers(player.agent)
    assert trained_rms and trained_rms.keys() == loaded_rms.keys()
    for name in trained_rms:
        assert torch.equal(trained_rms[name], loaded_rms[name]), name
    assert any(value.abs().sum() > 0 for value in trained_rms.values())
    player.run_playing_loop()
    assert player.step_count == 4
