"""The classic-control environments in their host form (no GPU): the library's host restatement of the kernels
(``cusrl_classic_step_cpu`` / ``cusrl_classic_reset_cpu``, the same ``__host__ __device__`` bodies) against a float64 evaluation of
the formulas, the reset contract, the environment classes and their checkpoint.  The kernels: tests/test_classic_control_gpu.py."""

import pytest
import torch

from _classic_control import (
    HOST_ERROR, TASKS, assert_exact_parts, inputs, reference_step, reset_cases, run_step, step_error,
)

NAMES = tuple(TASKS)


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.fixture(scope="module")
def references():
    return {name: reference_step(name, *inputs(name)) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_keep_clear_of_every_threshold(references, name):
    """Condition of the check: every test state sits farther from each termination threshold (and from the wall branch of
    MountainCar), in the float64 evaluation, than the widest asserted bound (4 x the measured host error, the GPU test's), so no
    flag may legitimately differ.  No row is left out."""
    reference = references[name]
    assert reference["margin"].shape == (inputs(name)[0].shape[0],)
    assert reference["margin"].min() > 4 * HOST_ERROR[name], (name, reference["margin"].min(), int(reference["margin"].argmin()))
    # the table does reach what it is there for
    assert reference["truncated"].any() and (name == "Pendulum" or reference["terminated"].any())
    saturated = reference["saturated"].any(axis=0)  # Pendulum: theta'; MountainCar: position and velocity
    assert {"CartPole": True, "Pendulum": saturated[-1], "MountainCar": saturated.all()}[name]


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_against_float64(cusrl, references, name):
    """``cusrl_classic_step_cpu`` within 2 x its measured error of the float64 formulas (the measurement: HOST_ERROR in
    tests/_classic_control.py and DESIGN.md §7); flags and step counter exact; saturated clamps exactly their bound."""
    from cusrl_amd import ops

    state, action, steps, max_steps = inputs(name)
    result = run_step(ops.classic_step_cpu, name, state, action, steps, max_steps)
    reference = references[name]
    error = step_error(result, reference)
    print(f"{name}: host restatement vs float64, scaled error {error:.3e} (asserted {2 * HOST_ERROR[name]:.1e})")
    assert_exact_parts(result, reference, name)
    assert error <= 2 * HOST_ERROR[name], (name, error)
    mask = torch.from_numpy(reference["saturated"])
    assert torch.equal(result["state"][mask], torch.from_numpy(reference["state"]).float()[mask]), name
    assert result["observation"].shape == (state.shape[0], TASKS[name]["O"]) and result["reward"].shape == (state.shape[0], 1)
    assert result["terminated"].dtype == torch.bool and result["truncated"].dtype == torch.bool


def test_ties_take_the_first_maximal_column(cusrl):
    from cusrl_amd import ops

    state = torch.zeros(4, 4)
    action = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    out = run_step(ops.classic_step_cpu, "CartPole", state, action, torch.zeros(4, dtype=torch.int32), 500)
    assert torch.equal(out["state"][0], out["state"][1]) and torch.equal(out["state"][0], out["state"][3])  # pushed left
    assert out["state"][0, 1] < 0 < out["state"][2, 1]
    state = torch.tensor([[-0.5, 0.0]]).repeat(4, 1)
    action = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [1.0, 1.0, 3.0], [5.0, 1.0, 5.0]])
    out = run_step(ops.classic_step_cpu, "MountainCar", state, action, torch.zeros(4, dtype=torch.int32), 200)
    velocity = out["state"][:, 1]
    assert velocity[0] == velocity[3] < velocity[1] < velocity[2]


@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("name", NAMES)
def test_reset_contract_on_the_host(cusrl, name, N):
    from cusrl_amd import ops

    reset_cases(ops.classic_reset_cpu, name, torch.device("cpu"), N)


def test_argument_checks(cusrl):
    from cusrl_amd import _native, ops

    state, steps, episode = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="unknown classic-control task"):
        ops.classic_step_cpu("Acrobot", torch.zeros(3, 2), state, steps, 500)
    with pytest.raises(ValueError, match="'action'"):
        ops.classic_step_cpu("CartPole", torch.zeros(3, 3), state, steps, 500)
    with pytest.raises(ValueError, match="'steps'"):
        ops.classic_step_cpu("CartPole", torch.zeros(3, 2), state, steps.long(), 500)
    with pytest.raises(ValueError, match="'state'"):
        ops.classic_step_cpu("Pendulum", torch.zeros(3, 1), state, steps, 200)
    with pytest.raises(ValueError, match="'count'"):
        ops.classic_reset_cpu("CartPole", 1, torch.arange(3), torch.zeros(1, dtype=torch.int64), state, steps, episode, 500)
    with pytest.raises(_native.NativeError, match="code -1"):
        ops.classic_step_cpu("CartPole", torch.zeros(3, 2), state, steps, 0)
    # an id outside [0, N) is skipped: nothing is touched, its row is zeros
    state[:] = 0.5
    rows = ops.classic_reset_cpu("CartPole", 1, torch.tensor([7, -1, 1]), None, state, steps, episode, 500)
    assert (rows[:2] == 0).all() and episode.tolist() == [0, 1, 0] and (state[0] == 0.5).all() and torch.equal(rows[2], state[1])
    # N == 0 / no slots: nothing to do
    empty = ops.classic_step_cpu("CartPole", torch.zeros(0, 2), torch.zeros(0, 4), torch.zeros(0, dtype=torch.int32), 500)
    assert empty[0].shape == (0, 4)
    assert ops.classic_reset_cpu("CartPole", 1, torch.zeros(0, dtype=torch.int64), None, state, steps, episode, 500).shape == (0, 4)


def test_environment_classes(cusrl):
    env = cusrl.environment
    with pytest.raises(ValueError, match="CartPole, Pendulum, MountainCar"):
        env.make("Acrobot", 4)
    for name, (observation_dim, action_dim) in {"CartPole": (4, 2), "Pendulum": (3, 1), "MountainCar": (2, 3)}.items():
        torch.manual_seed(5)
        e = env.make(name, 6, device="cpu")
        assert isinstance(e, cusrl.Environment) and type(e) is getattr(env, name)
        assert (e.observation_dim, e.action_dim, e.spec.reward_dim, e.spec.autoreset) == (observation_dim, action_dim, 1, False)
        assert not e.capturable and not e.generator_free and e.get_metrics() == {}  # (both True on a GPU: the GPU tests)
        generator_state = torch.get_rng_state()
        observation, state, info = e.reset(randomize_episode_progress=True)
        assert observation.shape == (6, observation_dim) and state is None and info == {}
        assert (e.episode == 1).all() and e.steps.unique().numel() > 1
        next_observation, state, reward, terminated, truncated, info = e.step(torch.zeros(6, action_dim))
        assert next_observation.shape == (6, observation_dim) and reward.shape == (6, 1) and state is None
        assert terminated.shape == truncated.shape == (6, 1) and terminated.dtype == torch.bool
        rows, _, _ = e.reset(indices=[4, 1])
        assert rows.shape == (2, observation_dim) and e.episode.tolist() == [1, 2, 1, 1, 2, 1]
        assert torch.equal(torch.get_rng_state(), generator_state)  # nothing is drawn from torch's generator
        # the seed follows torch.initial_seed() / seed=, as SyntheticEnvironment's stream does
        torch.manual_seed(5)
        assert torch.equal(env.make(name, 6, device="cpu").reset()[0], env.make(name, 6, device="cpu", seed=5).reset()[0])
        assert not torch.equal(env.make(name, 6, device="cpu", seed=6).reset()[0], env.make(name, 6, device="cpu", seed=5).reset()[0])
    short = env.CartPole(2, device="cpu", max_episode_steps=3)
    short.reset()
    flags = [short.step(torch.tensor([[0.0, 1.0], [1.0, 0.0]]))[4].flatten().tolist() for _ in range(3)]
    assert flags == [[False, False], [False, False], [True, True]]


@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_resumes_the_same_trajectories(cusrl, name):
    """``state_dict`` -> fresh env -> ``load_state_dict``: the next 20 steps under a fixed action sequence, resets of the finished
    envs included, are bit-identical to the original env's."""
    N, A = 16, TASKS[name]["A"]
    generator = torch.Generator().manual_seed(9)
    actions = [torch.randn(N, A, generator=generator) for _ in range(30)]
    original = cusrl.environment.make(name, N, device="cpu", seed=3, max_episode_steps=12)

    def advance(env, action):
        observation, _, reward, terminated, truncated, _ = env.step(action)
        done = (terminated | truncated).squeeze(-1).nonzero().squeeze(-1)
        rows = env.reset(indices=done)[0] if done.numel() else observation[:0]
        return observation, reward, terminated, truncated, rows

    original.reset(randomize_episode_progress=True)
    for action in actions[:10]:
        advance(original, action)
    checkpoint = original.state_dict()
    assert set(checkpoint) >= {"state", "steps", "episode", "seed"}
    resumed = cusrl.environment.make(name, N, device="cpu", seed=77, max_episode_steps=12)
    resumed.load_state_dict(checkpoint)
    state_address = resumed.state.data_ptr()
    resets = 0
    for action in actions[10:]:
        a, b = advance(original, action), advance(resumed, action)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        resets += a[4].shape[0]
    assert resets > 0 and resumed.state.data_ptr() == state_address  # (loaded in place: captured steps keep their addresses)
    assert torch.equal(original.state, resumed.state) and torch.equal(original.episode, resumed.episode)
    with pytest.raises(ValueError, match="cannot be loaded"):
        cusrl.environment.make("CartPole" if name != "CartPole" else "Pendulum", N, device="cpu").load_state_dict(checkpoint)


def test_the_golden_holds_its_own_condition(golden):
    """tests/golden/classic_control.npz (the reference's PPO on the host form of CartPole, three seeds): in every seed the mean
    over the last 5 iterations is at least 3 x the mean over the first 2."""
    g = golden("classic_control")
    curves = g["episode_length"]
    assert curves.shape == (3, int(g["num_iterations"]))
    assert (curves[:, -5:].mean(axis=1) >= 3 * curves[:, :2].mean(axis=1)).all()
    assert int(g["hyper.num_steps_per_update"]) == 32 and int(g["num_envs"]) == 64 and str(g["hyper.action_space_type"]) == "discrete"
