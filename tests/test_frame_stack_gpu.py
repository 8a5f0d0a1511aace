"""The frame-stack kernels on an MI355X: ``cusrl_frame_stack_push`` / ``cusrl_frame_stack_reset`` against their host restatements
bit for bit (16-byte and 4-byte paths on the same data, column tables, both paddings, fresh flags, device-side counts, a grid
whose stride loop turns), the launch census, ``environment.FrameStack`` around CartPole and Pendulum against the numpy
restatement of gymnasium's wrapper (tests/_frame_stack.py), the captured rollout against the host-driven loop, and the deployment
round trip through ``nn.ObservationStacker`` in front of a ``DeployedPolicy``."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _export as shared
from _frame_stack import DequeStack, expected, frames, offset_view, words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _columns(K0: int, seed: int) -> list[int]:
    """A permuting subset of ``[0, K0)`` (every column for ``K0 <= 2``)."""
    order = np.random.RandomState(seed).permutation(K0).tolist()
    return order[: max(1, (3 * K0 + 3) // 4)] if K0 > 2 else order


def _pair(host: torch.Tensor, offset: bool) -> torch.Tensor:
    device = host.to(DEV)
    return offset_view(device) if offset else device


def _check_pair(ops, N, S, K0, columns, padding, offset, seed):
    """One history through a reset of every env, a push, a push with fresh flags and three counted resets (count 0, 1, L as
    device tensors), on the device and on the host: the same bits in ``out`` and ``H`` after every call, and ``out == H``."""
    K = K0 if columns is None else len(columns)
    host_H = torch.from_numpy(frames(seed, N, S, K).copy())
    device_H = _pair(host_H, offset)
    host_table = ops.frame_stack_columns(columns, K0, "cpu")
    device_table = ops.frame_stack_columns(columns, K0, DEV)
    vector = columns is None and K % 4 == 0 and not offset
    assert (device_H.data_ptr() % 16 == 0) == (not offset)

    def same(device_out, host_out, label):
        assert torch.equal(words(device_out), words(host_out)), label
        assert torch.equal(words(device_H), words(host_H)), label
        assert device_out.untyped_storage().data_ptr() != device_H.untyped_storage().data_ptr(), label

    everyone = torch.arange(N, dtype=torch.int64)
    rows = torch.from_numpy(frames(seed + 1, N, K0))
    device_out = ops.frame_stack_reset(device_H, everyone.to(DEV), None, _pair(rows, offset), device_table, padding)
    same(device_out, ops.frame_stack_reset_cpu(host_H, everyone, None, rows, host_table, padding), "reset of every env")
    assert torch.equal(words(device_out), words(device_H).view(N, -1))
    obs = torch.from_numpy(frames(seed + 2, N, K0))
    out_buffer = _pair(torch.zeros(N, S * K), offset)  # (the 4-byte path needs every pointer off the boundary or any one of them)
    device_out = ops.frame_stack_push(device_H, _pair(obs, offset), device_table, None, padding, out=out_buffer)
    same(device_out, ops.frame_stack_push_cpu(host_H, obs, host_table, None, padding), "push")
    assert device_out is out_buffer and torch.equal(words(device_out), words(device_H).view(N, -1))
    fresh = torch.zeros(N, dtype=torch.bool)
    fresh[:: 3] = True
    device_fresh = fresh.to(DEV)
    obs = torch.from_numpy(frames(seed + 3, N, K0))
    device_out = ops.frame_stack_push(device_H, _pair(obs, offset), device_table, device_fresh, padding)
    same(device_out, ops.frame_stack_push_cpu(host_H, obs, host_table, fresh, padding), "push with fresh flags")
    assert not device_fresh.any() and not fresh.any()
    L = min(N, 5)
    generator = torch.Generator().manual_seed(seed)
    for count in (0, 1, L):
        ids = torch.randperm(N, generator=generator)[:L].to(torch.int64)
        if 1 <= count < L:
            ids[-1] = ids[0]  # a stale id that repeats the valid one: its row is dropped, the history is the valid slot's
        rows = torch.from_numpy(frames(seed + 4 + count, L, K0))
        device_count = torch.tensor([count], dtype=torch.int32, device=DEV)
        device_out = ops.frame_stack_reset(device_H, ids.to(DEV), device_count, _pair(rows, offset), device_table, padding)
        host_out = ops.frame_stack_reset_cpu(host_H, ids, torch.tensor([count], dtype=torch.int32), rows, host_table, padding)
        valid = ids[:count].tolist()
        keep = [j for j in range(L) if j < count or int(ids[j]) not in valid]  # (every row but the one the caller drops)
        assert torch.equal(words(device_out[keep]), words(host_out[keep])), ("counted reset", count)
        assert torch.equal(words(device_H), words(host_H)), ("counted reset", count)
    return vector


@pytest.mark.parametrize("padding", ["reset", "zero"])
@pytest.mark.parametrize("K0", [1, 3, 4, 8, 48])
@pytest.mark.parametrize("S", [1, 2, 4, 16])
def test_kernels_have_the_bits_of_their_host_restatements(cusrl, S, K0, padding):
    """N in {1, 3, 65, 257} (one lane, below a wave, just over a wave, just over a block) at every S and K: without a column table
    on 16-byte aligned buffers (the 16-byte path where K % 4 == 0), the same through views one float off the boundary (the 4-byte
    path on the same data), and with a permuting column table.  Frames hold NaNs with payloads, -0.0, +-Inf and a denormal."""
    from cusrl_amd import ops

    vector_cases = 0
    for N in (1, 3, 65, 257):
        seed = 1000 * S + 10 * K0 + N
        vector_cases += _check_pair(ops, N, S, K0, None, padding, False, seed)
        _check_pair(ops, N, S, K0, None, padding, True, seed)
        _check_pair(ops, N, S, K0, _columns(K0, seed), padding, False, seed)
    assert vector_cases == (4 if K0 % 4 == 0 else 0)


@pytest.mark.parametrize("vector", [False, True], ids=["4-byte", "16-byte"])
def test_the_stride_loops_turn(cusrl, vector):
    """At S = 2, more than twice as many column lanes as the capped grid has threads (2048 blocks of 256): the push kernel's tile
    loop and the reset kernel's lane loop both go round at least twice.  4-byte path: 4097 rows of 256 columns through a
    permutation (one row per tile); 16-byte path: 4097 rows of 1024 columns (256 lanes of four)."""
    from cusrl_amd import ops

    N, S, K = 4097, 2, 1024 if vector else 256
    assert N * (K // 4 if vector else K) > 2 * 2048 * 256
    columns = None if vector else np.random.RandomState(0).permutation(K).tolist()
    generator = torch.Generator().manual_seed(5)
    host_H, obs, rows = (torch.randn(shape, generator=generator) for shape in ((N, S, K), (N, K), (N, K)))
    for tensor in (host_H, obs, rows):
        tensor.view(-1)[:: 4099] = float("nan")
    device_H = host_H.to(DEV)
    host_table, device_table = ops.frame_stack_columns(columns, K, "cpu"), ops.frame_stack_columns(columns, K, DEV)
    fresh = torch.zeros(N, dtype=torch.bool)
    fresh[:: 5] = True
    device_fresh = fresh.to(DEV)
    device_out = ops.frame_stack_push(device_H, obs.to(DEV), device_table, device_fresh, "zero")
    host_out = ops.frame_stack_push_cpu(host_H, obs, host_table, fresh, "zero")
    assert torch.equal(words(device_out), words(host_out)) and torch.equal(words(device_H), words(host_H)) and not device_fresh.any()
    ids = torch.randperm(N, generator=generator)
    count = torch.tensor([N - 7], dtype=torch.int32)
    device_out = ops.frame_stack_reset(device_H, ids.to(DEV), count.to(DEV), rows.to(DEV), device_table, "reset")
    host_out = ops.frame_stack_reset_cpu(host_H, ids, count, rows, host_table, "reset")
    assert torch.equal(words(device_out), words(host_out)) and torch.equal(words(device_H), words(host_H))


def test_launch_census(cusrl):
    """One stacker call is one ``cusrl_frame_stack_push``; a wrapper step adds exactly one launch to the inner step, a reset one —
    by the call counter, and by the node list of a graph captured around them (kernel nodes only: no memset, no copy)."""
    from cusrl_amd import _native, ops

    def moved(before):
        return {key: value - before.get(key, 0) for key, value in _native.launch_counts.items() if value != before.get(key, 0)}

    stacker = cusrl.nn.ObservationStacker(48, 4).to(DEV)
    observation = torch.randn(64, 48, device=DEV)
    stacker(observation)  # (allocates the history)
    before = dict(_native.launch_counts)
    stacked = stacker(observation, done=torch.zeros(64, dtype=torch.bool, device=DEV))
    assert moved(before) == {"cusrl_frame_stack_push": 1} and stacked.shape == (64, 192)
    env = cusrl.environment.FrameStack(cusrl.environment.make("CartPole", 64, device=DEV, seed=1), 4, columns=[0, 2])
    assert env.capturable and env.generator_free
    action = torch.zeros(64, 2, device=DEV)
    indices = torch.arange(64, dtype=torch.int64, device=DEV)
    count = torch.tensor([5], dtype=torch.int32, device=DEV)
    before = dict(_native.launch_counts)
    env.reset()
    assert moved(before) == {"cusrl_classic_reset": 1, "cusrl_frame_stack_reset": 1}
    before = dict(_native.launch_counts)
    env.step(action)
    assert moved(before) == {"cusrl_classic_step": 1, "cusrl_frame_stack_push": 1}
    before = dict(_native.launch_counts)
    env.reset_static(indices, count)
    env.reset(indices=[3, 9])
    assert moved(before) == {"cusrl_classic_reset": 2, "cusrl_frame_stack_reset": 2}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for call, kernel in ((lambda: env.step(action), "frame_stack_push_kernel"),
                         (lambda: env.reset_static(indices, count), "frame_stack_reset_kernel")):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, stream=stream):
            call()
        census = ops.graph_census(graph)
        assert (census["kernel"], census["memcpy"], census["memset"], census["other"]) == (2, 0, 0, 0), census
        assert sum(kernel in name for name in census["names"]) == 1, census["names"]
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="device tensor"):
        ops.frame_stack_push(torch.zeros(2, 2, 2), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="CPU tensors"):
        cusrl.nn.ObservationStacker(4, 2)(torch.zeros(2, 4))  # (the gate is shut in a gpu test, as in a user's process)
    # an input the kernel does not take: the torch expression, in fp32, with the kernel's bits
    other = cusrl.nn.ObservationStacker(48, 4).to(DEV)
    native = cusrl.nn.ObservationStacker(48, 4).to(DEV)
    for step in range(3):
        observation = torch.randn(64, 48, device=DEV)
        strided = torch.stack([observation, observation], dim=-1)[..., 0]
        assert not strided.is_contiguous()
        assert torch.equal(words(other(strided.double() if step == 1 else strided)), words(native(observation)))


@pytest.mark.parametrize("static", [False, True], ids=["reset", "reset_static"])
@pytest.mark.parametrize("name,columns", [("CartPole", None), ("Pendulum", [0, 1])])
def test_wrapped_tasks_stack_what_the_tasks_observe(cusrl, name, columns, static):
    """8 envs, fixed actions, 40 steps: at every step the wrapper's observation is the stack the numpy restatement builds from the
    task's own observation sequence — the task run a second time, unwrapped, from the same seed — through the resets that happen on
    the way (CartPole's poles fall under a constant push; Pendulum is truncated after 15 steps), by ``reset(indices=...)`` and by
    ``reset_static`` with a device-side count."""
    N, S = 8, 4
    kwargs = dict(device=DEV, seed=11, max_episode_steps=15 if name == "Pendulum" else None)
    env = cusrl.environment.FrameStack(cusrl.environment.make(name, N, **kwargs), S, columns=columns)
    twin = cusrl.environment.make(name, N, **kwargs)
    reference = DequeStack(N, S, "reset", columns)
    observation = env.reset(randomize_episode_progress=True)[0]
    twin_observation = twin.reset(randomize_episode_progress=True)[0].cpu().numpy()
    for e in range(N):
        reference.reset(e, twin_observation[e])
    assert torch.equal(words(observation), expected(reference.rows()))
    generator = torch.Generator().manual_seed(3)
    action = torch.randn(N, env.action_dim, generator=generator).to(DEV)  # fixed: the same rows at every step
    resets = 0
    for t in range(40):
        stacked, _, reward, terminated, truncated, _ = env.step(action)
        twin_step = twin.step(action)
        raw = twin_step[0].cpu().numpy()
        for e in range(N):
            reference.step(e, raw[e])
        assert torch.equal(words(stacked), expected(reference.rows())), t
        assert torch.equal(reward, twin_step[2]) and torch.equal(terminated, twin_step[3]) and torch.equal(truncated, twin_step[4])
        done = (terminated | truncated).squeeze(-1)
        ids = done.nonzero().squeeze(-1)
        if static:
            indices = torch.zeros(N, dtype=torch.int64, device=DEV)
            indices[: ids.numel()] = ids
            count = torch.tensor([ids.numel()], dtype=torch.int32, device=DEV)
            rows, twin_rows = env.reset_static(indices, count)[0], twin.reset_static(indices, count)[0]
        elif ids.numel():
            rows, twin_rows = env.reset(indices=ids)[0], twin.reset(indices=ids)[0]
        for j, e in enumerate(ids.tolist()):
            reference.reset(e, twin_rows[j].cpu().numpy())
            assert torch.equal(words(rows[j]), expected(reference.row(e))), (t, e)
        resets += ids.numel()
        assert torch.equal(words(env.history).view(N, -1), expected(reference.rows())), t
    assert resets >= N  # every env restarted at least once on average
    assert torch.equal(env.env.state, twin.state) and torch.equal(env.env.episode, twin.episode)


def _train(cusrl, capture, T):
    cusrl.set_global_seed(21)
    env = cusrl.environment.FrameStack(cusrl.environment.make("CartPole", 8, device=DEV, max_episode_steps=16), 4)
    factory = cusrl.preset.PpoAgentFactory(
        num_steps_per_update=T, sampler_epochs=2, sampler_mini_batches=2, compile=True, actor_hidden_dims=(64, 64),
        critic_hidden_dims=(64, 64), activation_fn="Tanh", action_space_type="discrete", optimizer_kwargs={"capturable": True, "fused": True})
    trainer = cusrl.Trainer(env, factory, num_iterations=4, verbose=False)
    trainer.capture_rollout = capture
    trainer.run_training_loop()
    return trainer


def test_captured_rollout_is_bit_identical_to_the_host_driven_loop(cusrl):
    """``FrameStack(CartPole(8), 4)``, T = 8, the small ``ppo`` preset with ``compile=True``, host-driven against captured from the
    same seed, in the form tests/test_captured_rollout.py and tests/test_classic_control_gpu.py use for bare envs.  Four
    iterations, not two: the driver runs iteration 0 host-driven and iteration 1 eagerly on the capture stream, captures one graph
    per step in iteration 2 and the whole rollout as one graph in iteration 3 — after two iterations nothing has been captured and
    the counter asserted here (``graphed.captured == T``) is still 0."""
    T = 8
    host, captured = _train(cusrl, False, T), _train(cusrl, True, T)
    assert host._graphed_rollout is None and host._static_resets
    graphed = captured._graphed_rollout
    assert graphed is not None and graphed.captured == T and len(graphed.rollouts) == 1, (graphed and graphed.captured)
    a, b = host.agent, captured.agent
    assert set(a.buffer.storage) == set(b.buffer.storage)
    for key in a.buffer.storage:
        assert torch.equal(a.buffer.storage[key], b.buffer.storage[key]), key
    assert a.buffer["observation"].shape[-1] == 16
    for (parameter_name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), parameter_name
    for attr in ("episode_rew", "episode_len", "rew_buffer", "len_buffer"):
        assert torch.equal(getattr(host.stats, attr), getattr(captured.stats, attr)), attr
    assert host.stats.num_episodes == captured.stats.num_episodes and host.stats.num_episodes > 0
    assert torch.equal(words(host.environment.history), words(captured.environment.history))
    for attr in ("state", "steps", "episode"):
        assert torch.equal(getattr(host.environment.env, attr), getattr(captured.environment.env, attr)), attr
    assert (host.environment.env.episode > 1).all() and (a.buffer["terminated"].any() or a.buffer["truncated"].any())
    # the stored observations are stacks: in a transition that did not end an episode, the three newest frames of `observation`
    # are the three oldest of `next_observation`
    observation, following = a.buffer["observation"], a.buffer["next_observation"]
    assert torch.equal(observation[..., 4:], following[..., :12])


def test_deployment_round_trip(cusrl, tmp_path):
    """Two updates on ``FrameStack(Pendulum(8), 4)``, ``agent.export``; then over 12 steps of the wrapped task (episodes of 5
    steps, started at random progress) ``DeployedPolicy(stacker(raw observation))`` against the agent's own deterministic act on
    the wrapper's stacked observation: the stacker rebuilds the wrapper's observation bit for bit from the raw one and the done
    flags, and the actions agree to the tolerance tests/test_export_gpu.py uses for the same comparison."""
    from cusrl_amd import _native

    N, S = 8, 4
    cusrl.set_global_seed(9)
    make = lambda: cusrl.environment.make("Pendulum", N, device=DEV, seed=4, max_episode_steps=5)  # noqa: E731
    env = cusrl.environment.FrameStack(make(), S)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=1, sampler_mini_batches=2, normalize_observation=True,
                                           device=DEV)
    trainer = cusrl.Trainer(env, factory, num_iterations=2, verbose=False)
    trainer.run_training_loop()
    agent = trainer.agent
    policy = cusrl.DeployedPolicy.load(agent.export(tmp_path), map_location=DEV)
    assert policy.observation_dim == env.observation_dim == S * 3
    agent.set_inference_mode(True, deterministic=True)
    env, twin = cusrl.environment.FrameStack(make(), S), make()
    stacker = cusrl.nn.ObservationStacker(3, S).to(DEV)
    # the scripted sequence: what the wrapper shows the agent, what the task itself shows, and which envs finish with that step
    observation, raw = env.reset(randomize_episode_progress=True)[0], twin.reset(randomize_episode_progress=True)[0]
    script, restarts = [], 0
    for t in range(12):
        expected_action = agent.act(observation.clone())
        following, _, _, terminated, truncated, _ = env.step(expected_action)
        following_raw = twin.step(expected_action)[0]
        done = (terminated | truncated).squeeze(-1)
        script.append((raw.clone(), observation.clone(), expected_action.clone(), done.clone()))
        ids = done.nonzero().squeeze(-1)
        if ids.numel():
            following[ids] = env.reset(indices=ids)[0]
            following_raw[ids] = twin.reset(indices=ids)[0]
            restarts += ids.numel()
        observation, raw = following, following_raw
    assert restarts >= N
    before = _native.launch_counts.get("cusrl_frame_stack_push", 0)
    for t, (raw, observation, expected_action, done) in enumerate(script):
        if t % 2:  # a call with done= is a call followed by reset(done)
            stacked = stacker(raw, done=done)
        else:
            stacked = stacker(raw)
            stacker.reset(done)
        assert torch.equal(words(stacked), words(observation)), t
        assert shared.relative_to_largest(policy(stacked), expected_action) <= shared.PARITY, t
    assert _native.launch_counts["cusrl_frame_stack_push"] - before == len(script)
