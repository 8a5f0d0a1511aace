"""Player, Trial, Logger, SaveTransition and InferenceWrapper without a GPU (``CUSRL_HOST_FORMS`` is set by conftest).

The reference's ``Player`` imports on the generating machine, so ``tests/golden/player.npz`` is its own output
(tests/golden/make_player_golden.py); the loop is not restated."""

from __future__ import annotations

import json
import os
import signal

import numpy as np
import pytest
import torch

import cusrl_amd as cusrl
from cusrl_amd import _native, ops

import _player

METRICS = ("Mean step reward", "Mean episode reward", "Mean episode length")
RUNS = {"run1": dict(num_steps=12), "run2": dict(num_episodes=2), "run3": dict(num_episodes=1)}


def scripted(g):
    Environment, Agent = _player.scripted_classes(cusrl)
    environment = Environment(g["reward"], g["terminated"], g["truncated"])
    return environment, Agent(environment.spec)


class Trajectory(cusrl.Player.Hook):
    """``episode_count`` after every step (``step`` runs before the step's resets are counted, hence one step late + close)."""

    def __init__(self):
        self.counts = []

    def step(self, step, transition):
        if step:
            self.counts.append(self.player.episode_count.clone().numpy())

    def close(self):
        self.counts.append(self.player.episode_count.clone().numpy())


def test_exports_and_bindings():
    for name in ("Player", "PlayerHook", "Trial", "Logger", "LoggerFactory", "make_logger_factory", "InferenceWrapper"):
        assert name in cusrl.__all__ and hasattr(cusrl, name), name
    for name in ("Player", "PlayerHook", "PlayerHookComposite", "Trial", "Logger", "LoggerFactory", "LoggerFactoryLike",
                 "make_logger_factory"):
        assert name in cusrl.template.__all__ and hasattr(cusrl.template, name), name
    assert cusrl.Player is cusrl.template.Player and cusrl.Player.Hook is cusrl.PlayerHook
    assert cusrl.hook.SaveTransition is cusrl.hook.player.SaveTransition and "SaveTransition" in cusrl.hook.__all__
    assert cusrl.nn.InferenceWrapper is cusrl.InferenceWrapper and cusrl.Logger.Factory is cusrl.LoggerFactory
    assert callable(cusrl.utils.Rate) and callable(cusrl.utils.to_numpy)
    assert callable(ops.play_epilogue) and hasattr(cusrl.template.trainer.EnvironmentStats, "track_play")
    assert _native.ABI_VERSION == 7 and _player.SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    restype, argtypes = _native._PROTOTYPES["cusrl_play_epilogue"]
    assert restype is _native.c_int and argtypes[:16] == _native._PROTOTYPES["cusrl_step_epilogue"][1][:16] and len(argtypes) == 21
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.play_epilogue(*([torch.zeros(4, 1)] * 12), 0, torch.zeros(4, dtype=torch.int64), 1, torch.zeros(1, dtype=torch.int32),
                          torch.zeros(2, dtype=torch.int32))


def test_raw_entry_refuses_bad_arguments_without_a_gpu():
    _player.check_error_codes(_native.lib())


@pytest.mark.parametrize("run", list(RUNS))
def test_host_bookkeeping_reproduces_the_reference(golden, tmp_path, run, capsys):
    g = golden("player")
    environment, agent = scripted(g)
    trajectory = Trajectory()
    hooks = [trajectory]
    if run == "run3":
        hooks.append(cusrl.hook.SaveTransition(tmp_path / "transition", save_interval=4))
    player = cusrl.Player(environment, agent, hooks=hooks, progress_bar=False, device_bookkeeping=False, **RUNS[run])
    metrics = player.run_playing_loop()
    assert player.step_count == int(g[f"{run}_steps"]) and environment.closed == 1 and player.device_bookkeeping is False
    assert player.episode_count.dtype == torch.int64 and not player.episode_count.is_cuda
    assert np.array_equal(np.stack(trajectory.counts), g[f"{run}_episode_count"])
    for metric in METRICS:
        expected = g[f"{run}_{metric.lower().replace(' ', '_')}"]
        np.testing.assert_allclose(np.asarray(metrics[metric], np.float64), expected, rtol=1e-6, atol=0)
    assert "Mean episode length" in capsys.readouterr().out  # the table is printed
    if run == "run3":
        files = sorted(path.name for path in tmp_path.iterdir())
        assert files == list(g["run3_files"])
        for file in files:
            with np.load(tmp_path / file) as saved:
                assert set(saved.files) == set(cusrl.hook.SaveTransition.DEFAULT_KEYS)
                for key in saved.files:
                    expected = g[f"run3/{file}/{key}"]
                    assert saved[key].dtype == expected.dtype and np.array_equal(saved[key], expected), (file, key)


def test_default_bookkeeping_falls_back_to_the_host_on_a_cpu_env(golden):
    g = golden("player")
    environment, agent = scripted(g)
    player = cusrl.Player(environment, agent, num_steps=12, progress_bar=False)
    assert player.device_bookkeeping is None
    player.run_playing_loop()
    assert player.device_bookkeeping is False and player.step_count == 12
    assert np.array_equal(player.episode_count.numpy(), g["run1_episode_count"][-1])


def test_restated_kernel_agrees_with_the_reference_loop(golden):
    """The yardstick of the GPU tests against the reference: counters, the unfinished count that ends the loop and the ring in
    ascending env order, over the golden tables."""
    g = golden("player")
    reward, terminated, truncated = g["reward"], g["terminated"], g["truncated"]
    for run, target in (("run2", 2), ("run3", 1)):
        state = _player.EpilogueState(_player.N_ENVS, _player.REWARD_DIM, _player.N_ENVS)
        trajectory, parity, steps = [], 0, 0
        while True:
            row = steps % reward.shape[0]
            done, indices, unfinished = _player.play_epilogue_restated(state, reward[row], terminated[row], truncated[row], parity, target)
            assert np.array_equal(indices, np.flatnonzero(terminated[row] | truncated[row])) and np.all(np.diff(indices) > 0)
            parity ^= 1
            steps += 1
            trajectory.append(state.episode_count.copy())
            if unfinished == 0:
                break
        assert steps == int(g[f"{run}_steps"]) and np.array_equal(np.stack(trajectory), g[f"{run}_episode_count"])
        filled = min(int(state.counter[parity]), _player.N_ENVS)
        np.testing.assert_allclose(state.ring_rew[:filled].mean(axis=0), g[f"{run}_mean_episode_reward"], rtol=1e-6)
        np.testing.assert_allclose(state.ring_len[:filled].mean(), g[f"{run}_mean_episode_length"], rtol=1e-6)
        np.testing.assert_allclose(state.step_reward_sum / _player.N_ENVS / steps, g[f"{run}_mean_step_reward"], rtol=1e-5)
    # the recomputation the end-to-end GPU test holds the player to gives the same loop outcome from saved arrays alone
    T = int(g["run2_steps"]) + 5
    rows = np.arange(T) % reward.shape[0]
    steps, counts, metrics, _ = _player.recompute_play(reward[rows], (terminated | truncated)[rows], 2, _player.N_ENVS)
    assert steps == int(g["run2_steps"]) and np.array_equal(counts, g["run2_episode_count"][-1])
    np.testing.assert_allclose(metrics["Mean episode reward"], g["run2_mean_episode_reward"], rtol=1e-6)
    np.testing.assert_allclose(metrics["Mean step reward"], g["run2_mean_step_reward"], rtol=1e-5)


# ------------------------------------------------------------------------------------------------ hooks, close, SIGINT
def test_composite_order_close_on_error_and_sigint(golden):
    g = golden("player")
    calls = []

    class Named(cusrl.PlayerHook):
        def __init__(self, name, fail_at=None, interrupt_at=None):
            self.name, self.fail_at, self.interrupt_at = name, fail_at, interrupt_at

        def init(self, player):
            super().init(player)
            calls.append(("init", self.name))

        def step(self, step, transition):
            calls.append(("step", self.name, step))
            if step == self.fail_at:
                raise KeyError("boom")
            if step == self.interrupt_at:
                os.kill(os.getpid(), signal.SIGINT)

        def reset(self, indices):
            calls.append(("reset", self.name, list(indices)))

        def close(self):
            calls.append(("close", self.name))

    environment, agent = scripted(g)
    player = cusrl.Player(environment, agent, num_steps=3, progress_bar=False, hooks=[Named("a")], device_bookkeeping=False)
    assert player.register_hook(Named("b")) is player and isinstance(player.hook, cusrl.template.PlayerHookComposite)
    assert player.hook[0].player is player and player.hook[0].agent is agent and player.hook[1].environment is environment
    player.run_playing_loop()
    assert calls[:2] == [("init", "a"), ("init", "b")] and calls[-2:] == [("close", "a"), ("close", "b")]
    per_event = [c for c in calls if c[0] in ("step", "reset")]
    assert all(x[1] == "a" and y[1] == "b" and x[0] == y[0] and x[2:] == y[2:] for x, y in zip(per_event[::2], per_event[1::2]))
    done0 = np.flatnonzero(g["terminated"][0] | g["truncated"][0]).tolist()
    if done0:
        assert ("reset", "a", done0) in calls

    calls.clear()
    environment, agent = scripted(g)
    player = cusrl.Player(environment, agent, num_steps=5, progress_bar=False, hooks=[Named("x", fail_at=1)], device_bookkeeping=False)
    with pytest.raises(KeyError, match="boom"):
        player.run_playing_loop()
    assert calls[-1] == ("close", "x") and environment.closed == 1

    calls.clear()
    environment, agent = scripted(g)
    before = signal.getsignal(signal.SIGINT)
    player = cusrl.Player(environment, agent, progress_bar=False, hooks=[Named("s", interrupt_at=2)], device_bookkeeping=False)
    player.run_playing_loop()  # no limit at all: only the flag ends it, after the step in which it was raised
    assert player.interrupted and player.step_count == 3 and signal.getsignal(signal.SIGINT) is before


def test_save_transition_arguments(tmp_path):
    hook = cusrl.hook.SaveTransition(tmp_path / "data")
    assert hook.output_path == tmp_path / "data.npz" and hook.keys == cusrl.hook.SaveTransition.DEFAULT_KEYS
    assert cusrl.hook.SaveTransition(tmp_path / "data.npz").output_path == tmp_path / "data.npz"
    assert cusrl.hook.SaveTransition().output_path.name.startswith("transition_")
    Environment, Agent = _player.scripted_classes(cusrl)
    environment = Environment(*_player.make_tables())
    with pytest.raises(ValueError, match="save_interval"):
        cusrl.Player(environment, Agent(environment.spec), hooks=[cusrl.hook.SaveTransition(tmp_path / "x", save_interval=0)])
    # one file without an interval; numpy values take the reference's path
    hook = cusrl.hook.SaveTransition(tmp_path / "single", keys=("a",))
    hook.init(cusrl.Player(environment, Agent(environment.spec)))
    hook.step(0, {"a": np.arange(3)})
    hook.step(1, {"a": torch.arange(3)})
    hook.close()
    hook.close()  # nothing buffered: nothing written
    assert sorted(p.name for p in tmp_path.iterdir()) == ["single.npz"]
    assert np.array_equal(np.load(tmp_path / "single.npz")["a"], np.stack([np.arange(3)] * 2))


# ------------------------------------------------------------------------------------------------ Trial
def make_trial(root, experiment="Env_Algo", trial="t1", iterations=(0, 10, 2), metadata=None):
    home = root / experiment / trial
    (home / "ckpt").mkdir(parents=True)
    for i in iterations:
        torch.save({"iteration": i}, home / "ckpt" / f"ckpt_{i}.pt")
    (home / "ckpt" / "notes.txt").write_text("not a checkpoint")
    if metadata is not None:
        (home / "info" / "trial").mkdir(parents=True)
        (home / "info" / "trial" / "metadata.json").write_text(json.dumps(metadata))
    return home


def test_trial_paths_names_metadata_and_errors(tmp_path, capsys):
    Trial = cusrl.Trial
    old = make_trial(tmp_path, trial="2024-01-01_a", iterations=(5,))
    new = make_trial(tmp_path, trial="2024-01-02_b", metadata={"seed": 3})
    (tmp_path / "Env_Algo" / "latest").symlink_to(old.name, target_is_directory=True)  # NOT the newest name: the link decides

    by_experiment = Trial(tmp_path / "Env_Algo")
    assert by_experiment.home == old.resolve() and by_experiment.iteration == 5 and by_experiment.metadata == {}
    assert "Trial loaded from" in capsys.readouterr().out
    by_trial = Trial(new, verbose=False)
    assert capsys.readouterr().out == ""
    assert by_trial.home == new.absolute() and by_trial.all_iterations == [0, 2, 10] and by_trial.iteration == 10
    assert by_trial.name == "2024-01-02_b" and by_trial.metadata == {"seed": 3}
    assert (by_trial.experiment_name, by_trial.environment_name, by_trial.algorithm_name) == ("Env_Algo", "Env", "Algo")
    assert by_trial.checkpoint_path == new.absolute() / "ckpt/ckpt_10.pt" and by_trial.load_checkpoint() == {"iteration": 10}
    by_file = Trial(new / "ckpt" / "ckpt_2.pt", verbose=False)
    assert by_file.home == new.absolute() and by_file.iteration == 2 and by_file.load_checkpoint(map_location="cpu") == {"iteration": 2}

    legacy = Trial(make_trial(tmp_path, experiment="Env:Algo"), verbose=False)
    assert (legacy.experiment_name, legacy.environment_name, legacy.algorithm_name) == ("Env:Algo", "Env", "Algo")
    other = Trial(make_trial(tmp_path, experiment="My_Env_Algo"), verbose=False)
    assert other.experiment_name is None and other.environment_name is None and other.algorithm_name is None

    with pytest.raises(FileNotFoundError, match="does not exist"):
        Trial(tmp_path / "missing")
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError, match="not a valid trial directory"):
        Trial(tmp_path / "empty")
    (tmp_path / "empty" / "ckpt").mkdir()
    with pytest.raises(FileNotFoundError, match="No checkpoint files"):
        Trial(tmp_path / "empty")
    with pytest.raises(ValueError, match="not a valid checkpoint file"):
        Trial(new / "ckpt" / "notes.txt")


# ------------------------------------------------------------------------------------------------ Logger
def test_logger_layout_symlink_interval_and_factories(tmp_path):
    first = cusrl.Logger(tmp_path, name="run")
    stamp, _, name = first.log_dir.name.rpartition("_")
    assert name == "run" and len(stamp.split("-")) == 6 and first.log_dir.parent == tmp_path.absolute()
    assert first.info_dir.is_dir() and first.ckpt_dir.is_dir() and os.environ["TRIAL_LOG_DIR"] == str(first.log_dir)
    latest = tmp_path / "latest"
    assert latest.is_symlink() and os.readlink(latest) == first.log_dir.name
    second = cusrl.Logger.Factory(tmp_path, name="other", add_datetime_prefix=False)()
    assert second.log_dir == tmp_path.absolute() / "other" and os.readlink(latest) == "other"
    assert cusrl.Logger(tmp_path, name="", add_datetime_prefix=False).log_dir == tmp_path.absolute()
    bare = cusrl.Logger(tmp_path / "bare", name=None)
    assert bare.log_dir == (tmp_path / "bare").absolute() and not (tmp_path / "bare" / "latest").exists() and bare.ckpt_dir.is_dir()
    with pytest.raises(ValueError, match="must not contain"):
        cusrl.Logger(tmp_path, name="a/b")

    second.save_checkpoint({"x": 1}, iteration=7)
    assert torch.load(second.ckpt_dir / "ckpt_7.pt") == {"x": 1} and cusrl.Trial(tmp_path, verbose=False).iteration == 7
    second.save_info("hello", "trial/notes.txt")
    assert (second.info_dir / "trial" / "notes.txt").read_text() == "hello"

    logged = []

    class Recording(cusrl.Logger):
        def _log_impl(self, data, iteration):
            logged.append((dict(data), iteration))

    recording = Recording(tmp_path / "rec", name=None, interval=3)
    for i in range(7):
        recording.log({"a": float(i), **({"b": 10.0} if i % 2 else {})}, i + 1)
    assert logged == [({"a": 1.0, "b": 10.0}, 3), ({"a": 4.0, "b": 10.0}, 6)] and len(recording.data_list) == 1
    every = Recording(tmp_path / "rec1", name=None)
    every.log({"a": 2.0}, 1)
    assert logged[-1] == ({"a": 2.0}, 1)

    assert cusrl.make_logger_factory(None, None) is None and cusrl.make_logger_factory("recording") is None
    for kind in (None, "none", "None"):
        factory = cusrl.make_logger_factory(kind, tmp_path / "made", name="n", interval=2, add_datetime_prefix=False)
        assert type(factory) is cusrl.LoggerFactory and factory.interval == 2 and type(factory()) is cusrl.Logger
    # a subclass is found by its lower-cased name and asked for ITS factory (Logger's own unless it defines one)
    assert type(cusrl.make_logger_factory("Recording", tmp_path / "made2", name=None)) is cusrl.LoggerFactory
    with pytest.raises(KeyError):
        cusrl.make_logger_factory("tensorboard-of-nobody", tmp_path / "made3")


# ------------------------------------------------------------------------------------------------ InferenceWrapper, Rate
def test_inference_wrapper_formats_and_memory():
    torch.manual_seed(0)
    mlp = cusrl.Mlp(4, [8], 3)
    wrapper = cusrl.InferenceWrapper(mlp)
    assert wrapper.wrapped is mlp and (wrapper.input_dim, wrapper.output_dim, wrapper.is_recurrent) == (4, 3, False)
    x = np.random.RandomState(0).standard_normal((5, 4)).astype(np.float32)
    y = wrapper(x)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (5, 3)
    with torch.no_grad():
        assert np.array_equal(y, mlp.layers(torch.from_numpy(x)).numpy())
    y64 = wrapper(x.astype(np.float64))
    assert y64.dtype == np.float64 and np.array_equal(y64, y.astype(np.float64))
    one = wrapper(x[0])
    assert one.shape == (3,) and np.allclose(one, y[0], rtol=1e-6, atol=1e-7)
    t = wrapper(torch.from_numpy(x).double())
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.requires_grad and wrapper.memory is None

    gru = cusrl.InferenceWrapper(cusrl.Gru(4, 6))
    assert gru.is_recurrent and gru.memory is None
    first = gru(x)
    memory = gru.memory.clone()
    assert memory.shape == (5, 6) and memory.abs().sum() > 0
    second = gru(x)
    assert not np.array_equal(first, second) and not torch.equal(gru.memory, memory)  # the memory went into the second call
    kept = gru.memory.clone()
    gru.reset([1, 3])
    assert (gru.memory[[1, 3]] == 0).all() and torch.equal(gru.memory[[0, 2, 4]], kept[[0, 2, 4]])
    gru.reset()
    assert (gru.memory == 0).all()


def test_rate_and_to_numpy():
    import time

    with pytest.raises(ValueError):
        cusrl.utils.Rate(0)
    with pytest.raises(ValueError):
        cusrl.utils.Rate(10, threshold=-1)
    rate = cusrl.utils.Rate(1e6)  # a microsecond period: tick never sleeps noticeably
    assert rate.dt == 1e-6
    rate.last_time = time.perf_counter() - 10.0
    rate.tick()
    assert time.perf_counter() - rate.last_time < 1.0  # anchored at most `threshold` behind real time
    array = np.arange(3)
    assert cusrl.utils.to_numpy(array) is array and cusrl.utils.to_numpy([1, 2]).tolist() == [1, 2]
    assert cusrl.utils.to_numpy(torch.ones(2, requires_grad=True)).tolist() == [1.0, 1.0]
