"""The classic-control kernels (``csrc/environment.hip``) on the GPU, all five tasks: against the float64 formulas and the
library's host restatement, a misaligned state, canary rows around every operand, the reset contract, the launch census, the
captured rollout against the host-driven loop, and the project's first learning test — PPO on the device-resident CartPole against
curves recorded from the reference (tests/golden/make_classic_control_golden.py).  The host form: tests/test_classic_control.py.
No row here holds a non-finite value: that run is host only."""

import ctypes

import numpy as np
import pytest
import torch

from _classic_control import (
    HOST_ERROR, RANDOM_ROWS, TASKS, TRIG_COLUMNS, assert_exact_parts, inputs, reference_step, reset_cases, run_step, step_error,
)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = tuple(TASKS)


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


@pytest.fixture(scope="module")
def references():
    """Per task: the inputs, the float64 evaluation and the host restatement's result, computed once."""
    from cusrl_amd import ops

    out = {}
    for name in NAMES:
        state, action, steps, max_steps = inputs(name)
        out[name] = dict(inputs=(state, action, steps, max_steps), float64=reference_step(name, state, action, steps, max_steps),
                         host=run_step(ops.classic_step_cpu, name, state, action, steps, max_steps))
    return out


def _rows(reference: dict, rows: slice) -> dict:
    return {key: value[rows] for key, value in reference.items()}


def _device_step(name, state, action, steps, max_steps):
    from cusrl_amd import ops

    return run_step(ops.classic_step, name, state.to(DEV), action.to(DEV), steps.to(DEV), max_steps)


def _assert_against_both(name, result, float64, host):
    error = step_error(result, float64)
    print(f"{name}: kernel vs float64, scaled error {error:.3e} (asserted {4 * HOST_ERROR[name]:.1e}), rows {result['state'].shape[0]}")
    assert_exact_parts(result, float64, name)  # flags and step counter as the formulas give them ...
    # ... and everything without a transcendental in front of it, the host form's bits: flags, counter, the rewards that are a
    # function of the flag.  MountainCarContinuous's reward is too wherever the flag agrees: 100 or 0 minus 0.1 a a.
    for key in ("terminated", "truncated", "steps", "reward"):
        assert torch.equal(result[key].cpu(), host[key]), (name, key)
    mask = torch.from_numpy(float64["saturated"])
    assert torch.equal(result["state"].cpu()[mask], host["state"][mask]), name  # a clamp that saturates is its bound
    assert error <= 4 * HOST_ERROR[name], (name, error)
    return error


@pytest.mark.parametrize("rows", [1, 3, RANDOM_ROWS, "all"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_float64_and_the_host_restatement(cusrl, references, name, rows):
    """N = 1 and 3 (the head of the table), 257 (the random rows: two blocks) and the whole input set in one launch."""
    state, action, steps, max_steps = references[name]["inputs"]
    select = slice(None) if rows == "all" else (slice(-RANDOM_ROWS, None) if rows == RANDOM_ROWS else slice(0, rows))
    result = _device_step(name, state[select], action[select], steps[select], max_steps)
    _assert_against_both(name, result, _rows(references[name]["float64"], select), _rows(references[name]["host"], select))


@pytest.mark.parametrize("name", NAMES)
def test_a_state_one_float_off_a_16_byte_boundary_gives_the_same_bits(cusrl, references, name):
    """The scalar path of the kernel (state rows and, for Acrobot, the observation rows) against the vector path."""
    from cusrl_amd import ops

    state, action, steps, max_steps = references[name]["inputs"]
    M, S = state.shape
    aligned = _device_step(name, state, action, steps, max_steps)
    base = torch.zeros(M * S + 4, device=DEV)
    shifted = base[1 : 1 + M * S].view(M, S)
    shifted.copy_(state)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    device_steps = steps.to(DEV)
    outputs = ops.classic_step(name, action.to(DEV), shifted, device_steps, max_steps)
    result = dict(zip(("observation", "reward", "terminated", "truncated"), outputs), state=shifted, steps=device_steps)
    for key, value in aligned.items():
        assert torch.equal(result[key], value), (name, key)
    assert base[0] == 0 and (base[1 + M * S :] == 0).all()
    _assert_against_both(name, result, references[name]["float64"], references[name]["host"])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_a_launch_stays_inside_its_rows(cusrl, references, name, offset):
    """The C entry on over-allocated buffers, canary rows before and after every operand: rows outside [0, N) keep their bits, the
    rows inside equal the first launch's.  ``offset = 1``: the observation buffer starts one float further on, off the 8- or
    16-byte boundary its vector stores need, so the rows (Acrobot's 6-wide ones among them) go out as scalars — the same bits as
    the vector stores of ``offset = 0``.  (Pendulum's 3-wide rows are scalar stores at either offset.)"""
    from cusrl_amd import _native, ops

    state, action, steps, max_steps = references[name]["inputs"]
    first = _device_step(name, state, action, steps, max_steps)
    N, task, pad = state.shape[0], ops.CLASSIC_TASKS[name], 3

    def padded(rows: torch.Tensor, canary, shift=0):
        rows = rows.reshape(N, -1)
        width = rows.shape[1]
        flat = torch.full(((N + 2 * pad) * width + shift,), canary, dtype=rows.dtype, device=DEV)
        buffer = flat[shift:].view(N + 2 * pad, width)
        buffer[pad : pad + N] = rows.to(DEV)
        return buffer, flat

    buffers, flats = {}, {}
    for key, rows, canary, shift in (
            ("action", action, 7.5, 0), ("state", state, -3.25, 0), ("steps", steps, 12345, 0),
            ("observation", torch.zeros(N, task.observation_dim), 9.75, offset), ("reward", torch.zeros(N, 1), 6.5, 0),
            ("terminated", torch.zeros(N, 1, dtype=torch.uint8), 77, 0), ("truncated", torch.zeros(N, 1, dtype=torch.uint8), 78, 0)):
        buffers[key], flats[key] = padded(rows, canary, shift)
    before = {key: value.clone() for key, value in buffers.items()}
    inner = {key: value[pad:].data_ptr() for key, value in buffers.items()}
    odd = pad * task.observation_dim % 2  # (Pendulum alone: its 3 canary rows already end 4 bytes off)
    assert inner["observation"] % 8 == 4 * ((offset + odd) % 2) and inner["state"] % (4 * task.state_dim) == 0
    status = _native.lib().cusrl_classic_step(task.kind, inner["action"], inner["state"], inner["steps"], max_steps, inner["observation"],
                                              inner["reward"], inner["terminated"], inner["truncated"], N,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    for key, value in buffers.items():
        assert torch.equal(value[:pad], before[key][:pad]) and torch.equal(value[pad + N :], before[key][pad + N :]), (name, key)
    assert (flats["observation"][:offset] == 9.75).all()
    assert torch.equal(buffers["action"], before["action"])
    for key in ("state", "observation", "reward"):
        assert torch.equal(buffers[key][pad : pad + N], first[key].reshape(N, -1)), (name, key)
    assert torch.equal(buffers["steps"][pad : pad + N, 0], first["steps"])
    for key in ("terminated", "truncated"):
        assert torch.equal(buffers[key][pad : pad + N].bool(), first[key]), (name, key)


@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("name", NAMES)
def test_reset_contract_and_the_host_forms_bits(cusrl, name, N):
    """Every reset case on the device, and state / steps / episode / observation bit-identical to the host restatement's.  The one
    exception is stated in DESIGN.md §7: the observation columns that are cos / sin of a fresh angle (Pendulum's first two,
    Acrobot's first four) are the device's and not glibc's — those are held to the float64 values within the kernel bound instead
    (inside ``reset_cases``), the columns after them to the bits."""
    from cusrl_amd import ops

    device = reset_cases(ops.classic_reset, name, torch.device(DEV), N)
    host = reset_cases(ops.classic_reset_cpu, name, torch.device("cpu"), N)
    assert device.keys() == host.keys()
    trig = TRIG_COLUMNS.get(name, 0)
    for case in device:
        for index, (a, b) in enumerate(zip(device[case], host[case])):
            if isinstance(case, tuple) and index == 0:  # the observation rows
                assert torch.equal(a[:, trig:], b[:, trig:]), (name, case)
            else:
                assert torch.equal(a, b), (name, case, index)


@pytest.mark.parametrize("name", NAMES)
def test_launch_census(cusrl, name):
    """``step`` is exactly one ``cusrl_classic_step`` and ``reset_static`` exactly one ``cusrl_classic_reset``: by the call counter,
    and by the node list of a graph captured around them (one kernel node each, the task's own; no memset, no copy)."""
    from cusrl_amd import _native, ops

    env = cusrl.environment.make(name, 64, device=DEV, seed=1)
    assert env.capturable and env.generator_free
    env.reset()
    action = torch.zeros(64, env.action_dim, device=DEV)
    indices = torch.arange(64, dtype=torch.int64, device=DEV)
    count = torch.tensor([5], dtype=torch.int32, device=DEV)
    before = dict(_native.launch_counts)
    env.step(action)
    env.reset_static(indices, count)
    moved = {key: value - before.get(key, 0) for key, value in _native.launch_counts.items() if value != before.get(key, 0)}
    assert moved == {"cusrl_classic_step": 1, "cusrl_classic_reset": 1}, moved
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for call, kernel in ((lambda: env.step(action), "classic_step_kernel"), (lambda: env.reset_static(indices, count), "classic_reset_kernel")):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, stream=stream):
            call()
        census = ops.graph_census(graph)
        assert (census["kernel"], census["memcpy"], census["memset"], census["other"]) == (1, 0, 0, 0), census
        assert kernel in census["names"][0], census["names"]
    torch.cuda.synchronize()


def _train(cusrl, name, capture):
    T = 12
    cusrl.set_global_seed(21)
    env = cusrl.environment.make(name, 8, device=DEV, max_episode_steps=16)
    common = dict(num_steps_per_update=T, sampler_epochs=2, sampler_mini_batches=2, compile=True, actor_hidden_dims=(64, 64),
                  critic_hidden_dims=(64, 64), activation_fn="Tanh", optimizer_kwargs={"capturable": True, "fused": True})
    discrete = TASKS[name]["A"] > 1  # logits: CartPole, MountainCar, Acrobot; one torque or force: Pendulum, MountainCarContinuous
    factory = cusrl.preset.PpoAgentFactory(action_space_type="discrete" if discrete else "continuous", **common)
    trainer = cusrl.Trainer(env, factory, num_iterations=4, verbose=False)
    trainer.capture_rollout = capture
    trainer.run_training_loop()
    return trainer


@pytest.mark.parametrize("name", NAMES)
def test_captured_rollout_is_bit_identical_to_the_host_driven_loop(cusrl, name):
    """8 envs, 16-step episodes, 12-step rollouts, 4 iterations from the same seed, host-driven against ``compile=True`` capture:
    every buffer leaf, every parameter, the episode statistics and the env's own state / steps / episode — the envs with
    per-instance state that go through the ``reset_static`` contract.  The tasks with logits run the discrete preset, the other two
    the continuous one.  CartPole's poles do fall within 16 steps, Pendulum never terminates."""
    T = 12
    host, captured = _train(cusrl, name, False), _train(cusrl, name, True)
    assert host._graphed_rollout is None and host._static_resets
    graphed = captured._graphed_rollout
    assert graphed is not None and graphed.captured == T and len(graphed.rollouts) == 1, (graphed and graphed.captured)
    a, b = host.agent, captured.agent
    assert set(a.buffer.storage) == set(b.buffer.storage)
    for key in a.buffer.storage:
        assert torch.equal(a.buffer.storage[key], b.buffer.storage[key]), key
    for (parameter_name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), parameter_name
    for attr in ("episode_rew", "episode_len", "rew_buffer", "len_buffer"):
        assert torch.equal(getattr(host.stats, attr), getattr(captured.stats, attr)), attr
    assert host.stats.num_episodes == captured.stats.num_episodes and host.stats.num_episodes > 0
    for attr in ("state", "steps", "episode"):
        assert torch.equal(getattr(host.environment, attr), getattr(captured.environment, attr)), attr
    assert (host.environment.episode > 1).all() and (host.environment.steps <= 16).all()
    assert a.buffer["truncated"].any()
    if name in ("CartPole", "Pendulum"):
        assert a.buffer["terminated"].any() == (name == "CartPole")


def test_ppo_learns_cartpole_like_the_reference(cusrl, golden):
    """The `ppo` preset with the golden's hyper-parameters on the device-resident CartPole, as many iterations as the reference
    ran: the mean episode length over the last 5 iterations is at least half the reference's worst seed (seeds and random streams
    differ between the two implementations, three seeds give a rough spread) and at least 2 x its own first-2 mean.
    Measured on an MI355X: DESIGN.md §7."""
    g = golden("classic_control")
    iterations, num_envs = int(g["num_iterations"]), int(g["num_envs"])
    hyper = {key[len("hyper."):]: g[key].tolist() for key in g.files if key.startswith("hyper.")}
    hyper["actor_hidden_dims"], hyper["critic_hidden_dims"] = tuple(hyper["actor_hidden_dims"]), tuple(hyper["critic_hidden_dims"])
    reference_worst = float(g["episode_length"][:, -5:].mean(axis=1).min())

    class Curve(cusrl.Trainer.Hook):
        lengths = []

        def pre_log_info(self, info):
            self.lengths.append(info["Metric/episode_length"])

    cusrl.set_global_seed(0)
    env = cusrl.environment.CartPole(num_envs, device=DEV)
    curve = Curve()
    trainer = cusrl.Trainer(env, cusrl.preset.PpoAgentFactory(**hyper), num_iterations=iterations, verbose=False, hooks=[curve])
    trainer.run_training_loop()
    lengths = np.asarray(curve.lengths)
    assert lengths.shape == (iterations,)
    first, last = lengths[:2].mean(), lengths[-5:].mean()
    print(f"CartPole on the device: first-2 mean {first:.2f}, last-5 mean {last:.2f} (reference's worst seed {reference_worst:.2f}): "
          + " ".join(f"{v:.1f}" for v in lengths))
    assert last >= 0.5 * reference_worst, (last, reference_worst)
    assert last >= 2.0 * first, (last, first)
