"""Acrobot and MountainCarContinuous on the GPU (``csrc/environment.hip``): the kernels against the float64 formulas and the
library's host restatement, a misaligned state, canary rows around every operand (Acrobot's observation rows are 6 wide), the reset
contract, the launch census and the captured rollout against the host-driven loop.  The host form:
tests/test_classic_control_more.py.  No row here holds a non-finite value: that run is host only."""

import ctypes

import pytest
import torch

from _classic_control_more import (
    ACROBOT, HOST_ERROR, RANDOM_ROWS, TASKS, assert_exact_parts, inputs, reference_step, reset_cases, run_step, step_error,
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
    # ... and everything without a transcendental in front of it, the host form's bits: flags, counter, Acrobot's reward (a function
    # of its flag).  MountainCarContinuous's reward is too wherever the flag agrees: 100 or 0 minus 0.1 a a.
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
    rows inside equal the first launch's.  ``offset = 1``: the observation buffer starts one float off an 8-byte boundary, so
    Acrobot's 6-wide rows go out as scalars — the same bits as the 8-byte stores of ``offset = 0``."""
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
    assert inner["observation"] % 8 == 4 * offset and inner["state"] % (4 * task.state_dim) == 0
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
    """Every reset case on the device, and state / steps / episode / observation bit-identical to the host restatement's — except
    Acrobot's four observation columns cos / sin of the fresh angles, the device's and not glibc's: those are held to the float64
    values within the kernel bound instead (inside ``reset_cases``), its two velocity columns to the bits."""
    from cusrl_amd import ops

    device = reset_cases(ops.classic_reset, name, torch.device(DEV), N)
    host = reset_cases(ops.classic_reset_cpu, name, torch.device("cpu"), N)
    assert device.keys() == host.keys()
    for case in device:
        for index, (a, b) in enumerate(zip(device[case], host[case])):
            if name == ACROBOT and isinstance(case, tuple) and index == 0:  # the observation rows
                assert torch.equal(a[:, 4:], b[:, 4:]), (name, case)
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
    factory = cusrl.preset.PpoAgentFactory(action_space_type="discrete" if name == ACROBOT else "continuous", **common)
    trainer = cusrl.Trainer(env, factory, num_iterations=4, verbose=False)
    trainer.capture_rollout = capture
    trainer.run_training_loop()
    return trainer


@pytest.mark.parametrize("name", NAMES)
def test_captured_rollout_is_bit_identical_to_the_host_driven_loop(cusrl, name):
    """8 envs, 16-step episodes, 12-step rollouts, 4 iterations from the same seed, host-driven against ``compile=True`` capture:
    every buffer leaf, every parameter, the episode statistics and the env's own state / steps / episode.  Acrobot with the
    discrete preset, MountainCarContinuous with the continuous one."""
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
