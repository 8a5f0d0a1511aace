"""The five classic-control environments in their host form (no GPU): the condition on the inputs, Acrobot's formulas themselves in
float64, the library's host restatement of the kernels (``cusrl_classic_step_cpu`` / ``cusrl_classic_reset_cpu``, the same
``__host__ __device__`` bodies) against a float64 evaluation of the formulas, the reset contract, the environment classes, their
gym ids and their checkpoint.  The kernels: tests/test_classic_control_gpu.py."""

import numpy as np
import pytest
import torch

from _classic_control import (
    ACROBOT, CONTINUOUS, DT, HOST_ERROR, PI, RANDOM_ROWS, TASKS, acrobot_energy, acrobot_rk4, assert_exact_parts, inputs,
    reference_step, reset_cases, run_step, step_error,
)

NAMES = tuple(TASKS)
GYM_IDS = {"CartPole-v1": "CartPole", "Pendulum-v1": "Pendulum", "MountainCar-v0": "MountainCar", "Acrobot-v1": "Acrobot",
           "MountainCarContinuous-v0": "MountainCarContinuous"}


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.fixture(scope="module")
def references():
    return {name: reference_step(name, *inputs(name)) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_keep_clear_of_every_threshold(references, name):
    """Condition of the check: every test row sits farther, in the float64 evaluation, than the widest asserted bound (4 x the
    measured host error, the GPU test's) from each flag threshold, from the mountain cars' wall branch, from Acrobot's wrap
    boundaries (raw angle against +-pi) and from every clamp edge, so no flag, branch or saturation may legitimately differ.  No
    row is left out, and the table does reach what it is there for."""
    state, action, steps, max_steps = inputs(name)
    reference = references[name]
    table = state.shape[0] - RANDOM_ROWS
    assert reference["margin"].shape == (state.shape[0],)
    assert reference["margin"].min() > 4 * HOST_ERROR[name], (name, reference["margin"].min(), int(reference["margin"].argmin()))
    head = {key: value[:table] for key, value in reference.items()}
    assert head["truncated"].any()
    assert (~head["terminated"][:, 0] & (head["steps"] == max_steps - 1)).any()  # one short of the step limit: neither flag
    if name != "Pendulum":  # (which never terminates)
        assert head["terminated"].any()
        assert (head["terminated"][:, 0] & (head["steps"] == max_steps)).any()  # terminated at the step limit: not truncated
    saturated, new = reference["saturated"].any(axis=0), head["state"]
    if name == "Pendulum":
        assert saturated[-1]  # theta'
    elif name == ACROBOT:
        raw = head["raw"]
        for column in (0, 1):  # the raw angle leaves [-pi, pi] on either side
            assert (raw[:, column] > PI).any() and (raw[:, column] < -PI).any(), column
        for column, bound in ((2, 4 * PI), (3, 9 * PI)):  # each velocity bound in each direction
            assert (raw[:, column] > bound).any() and (raw[:, column] < -bound).any(), column
            assert (new[head["saturated"][:, column], column].__abs__() == bound).all()
        rest = (state[:table] == 0).all(dim=1).numpy()
        assert sorted(action[:table][rest].argmax(dim=1).tolist()) == [0, 1, 2]  # the hanging rest state with each torque
        assert (action[:table].max(dim=1).values[:, None] == action[:table]).sum(dim=1).max() >= 2  # tied logits
    elif name in ("MountainCar", CONTINUOUS):
        raw_p, raw_v = head["raw"].T
        assert saturated.all()  # position and velocity
        assert ((new[:, 0] == -1.2) & (raw_v < 0) & (new[:, 1] == 0)).any()  # the wall with v < 0
        assert (raw_v > 0.07).any() and (raw_v < -0.07).any() and (raw_p > 0.6).any()
        if name == CONTINUOUS:
            assert (action[:table, 0] > 1).any() and (action[:table, 0] < -1).any()
            assert ((new[:, 0] < 0.45) & (new[:, 0] > 0.4) & (new[:, 1] > 0)).any()  # stops short of the goal


def test_acrobot_formulas_conserve_energy_to_fourth_order():
    """The formulas themselves, float64 only (a transcription error shared by the C body and the float64 evaluation would pass
    every comparison between the two).  With zero torque the continuous system conserves
    ``E = 1/2 d1 w1^2 + d2 w1 w2 + 1/2 (m2 lc2^2 + I2) w2^2 - (m1 lc1 + m2 l1) g cos th1 - m2 lc2 g cos(th1 + th2)``: over 257
    states (theta in [-pi, pi], theta' in [-2, 2]) the largest |dE| of one 0.2 step of the unwrapped, unclamped Runge-Kutta step is
    at least 8 x that of two 0.1 steps (a fourth-order method predicts 16; measured with seed 0: 7.23e-3 against 4.80e-4, ratio
    15.1, at |E| up to 33).  With torque 1 the power fed in is ``theta2'``: ``dE / dt`` over dt = 0.001 equals it within 1e-2
    (measured 5.8e-3)."""
    rng = np.random.RandomState(0)
    s = np.concatenate([rng.uniform(-PI, PI, (RANDOM_ROWS, 2)), rng.uniform(-2, 2, (RANDOM_ROWS, 2))], axis=1)
    free = np.zeros(RANDOM_ROWS)
    energy = acrobot_energy(s)
    one = np.abs(acrobot_energy(acrobot_rk4(s, free, DT)) - energy).max()
    two = np.abs(acrobot_energy(acrobot_rk4(acrobot_rk4(s, free, DT / 2), free, DT / 2)) - energy).max()
    print(f"Acrobot, zero torque: |dE| {one:.3e} over one 0.2 step, {two:.3e} over two 0.1 steps, ratio {one / two:.1f}, "
          f"|E| up to {np.abs(energy).max():.1f}")
    assert two > 0 and one >= 8 * two, (one, two)
    assert one < 0.1  # (and the step does conserve it: a wrong term in f would move E by O(1) at |E| ~ 30)
    dt = 0.001
    power = (acrobot_energy(acrobot_rk4(s, np.ones(RANDOM_ROWS), dt)) - energy) / dt
    deviation = np.abs(power - s[:, 3]).max()
    print(f"Acrobot, torque 1: |dE/dt - theta2'| {deviation:.3e}")
    assert deviation <= 1e-2, deviation


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
    assert mask.any() == (name != "CartPole"), name  # (CartPole has no clamp)
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


def test_acrobot_ties_take_the_first_maximal_column(cusrl):
    from cusrl_amd import ops

    state = torch.tensor([[0.1, -0.2, 0.3, -0.4]]).repeat(5, 1)
    action = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [1.0, 1.0, 3.0], [5.0, 1.0, 5.0], [1.0, 0.0, 0.0]])
    out = run_step(ops.classic_step_cpu, ACROBOT, state, action, torch.zeros(5, dtype=torch.int32), 500)
    velocity = out["state"][:, 3]  # the torque acts on the second joint
    assert velocity[0] == velocity[3] == velocity[4] < velocity[1] < velocity[2]


def test_a_force_beyond_one_moves_the_car_like_one_and_costs_more(cusrl):
    """|a| > 1 on both sides: the state of a = +-1 to the bit, the reward of the RAW action."""
    from cusrl_amd import ops

    state = torch.tensor([[-0.5, 0.0]]).repeat(4, 1)
    action = torch.tensor([[1.7], [1.0], [-2.5], [-1.0]])
    out = run_step(ops.classic_step_cpu, CONTINUOUS, state, action, torch.zeros(4, dtype=torch.int32), 999)
    assert torch.equal(out["state"][0], out["state"][1]) and torch.equal(out["state"][2], out["state"][3])
    assert out["state"][0, 1] > 0 > out["state"][2, 1]
    expected = -0.1 * action.double() ** 2
    assert torch.allclose(out["reward"].double(), expected, rtol=0, atol=1e-7) and out["reward"][0] < out["reward"][1]


def test_non_finite_angles_step_on_the_host_and_return(cusrl):
    """The wrap has no loop: a state row holding NaN and Inf angles (and one far outside any range) steps and RETURNS, the
    non-finite angles come out non-finite, the huge one inside [-pi, pi] up to its own rounding, and the finite rows beside them
    are what they are alone.  (``while x > pi: x -= 2 pi`` would not return from the Inf row: on a GPU that is a hung card, so
    this run is host only.)"""
    from cusrl_amd import ops

    nan, inf = float("nan"), float("inf")
    state = torch.tensor([[nan, 0.0, 0.0, 0.0], [0.0, inf, 0.0, 0.0], [-inf, nan, 1.0, 1.0], [1.0e30, -1.0e30, 0.0, 0.0],
                          [1.0e4, -1.0e4, 0.0, 0.0], [0.1, -0.2, 0.3, -0.4]])
    action = torch.tensor([[0.0, 1.0, 0.0]]).repeat(6, 1)
    out = run_step(ops.classic_step_cpu, ACROBOT, state, action, torch.zeros(6, dtype=torch.int32), 500)
    angles = out["state"][:, :2]
    assert not torch.isfinite(angles[0, 0]) and not torch.isfinite(angles[1, 1]) and not torch.isfinite(angles[2]).any()
    assert (out["steps"] == 1).all()
    assert (angles[4].abs() <= PI + 1e-2).all()  # 1e4 is ~1600 turns: one ulp of it is 1e-3
    alone = run_step(ops.classic_step_cpu, ACROBOT, state[5:], action[5:], torch.zeros(1, dtype=torch.int32), 500)
    assert torch.equal(out["state"][5], alone["state"][0]) and torch.isfinite(out["observation"][5]).all()


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


def test_environment_classes_and_gym_ids(cusrl):
    from cusrl_amd import ops

    env = cusrl.environment

    for gym_id, cls in GYM_IDS.items():  # the same class by id for all five
        assert type(env.make(gym_id, 2, device="cpu")) is getattr(env, cls)
    for bare in ("Acrobot", "MountainCarContinuous"):  # the two later tasks have no bare name
        with pytest.raises(ValueError, match="CartPole, Pendulum, MountainCar"):
            env.make(bare, 4)
        with pytest.raises(ValueError, match="unknown classic-control task"):
            ops.classic_step_cpu(bare, torch.zeros(1, 1), torch.zeros(1, 2), torch.zeros(1, dtype=torch.int32), 10)
    assert list(ops.CLASSIC_TASKS) == ["CartPole", "Pendulum", "MountainCar", ACROBOT, CONTINUOUS]
    for name, (observation_dim, action_dim) in {ACROBOT: (6, 3), CONTINUOUS: (2, 1)}.items():
        torch.manual_seed(5)
        e = env.make(name, 6, device="cpu")
        assert isinstance(e, cusrl.Environment) and e.task is ops.CLASSIC_TASKS[name]
        assert (e.observation_dim, e.action_dim, e.spec.reward_dim, e.spec.autoreset) == (observation_dim, action_dim, 1, False)
        assert e.max_episode_steps == TASKS[name]["max_steps"] and tuple(e.state.shape) == (6, TASKS[name]["S"])
        assert not e.capturable and not e.generator_free
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
        torch.manual_seed(5)
        assert torch.equal(env.make(name, 6, device="cpu").reset()[0], env.make(name, 6, device="cpu", seed=5).reset()[0])
        assert not torch.equal(env.make(name, 6, device="cpu", seed=6).reset()[0], env.make(name, 6, device="cpu", seed=5).reset()[0])


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
    assert set(checkpoint) >= {"state", "steps", "episode", "seed"} and checkpoint["task"] == name
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
