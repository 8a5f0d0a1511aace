"""``cusrl_reward_normalize`` (``csrc/reward_norm.hip``) on the GPU: against the float64 restatement and the library's host
restatement, a misaligned reward, canary rows around every operand, repeated calls, the launch census, and the hook inside the
trainer: host-driven against the captured rollout, the raw episode return, a checkpoint.  The host form:
tests/test_reward_normalization.py.  No operand here holds a non-finite value: that run is host only."""

import ctypes

import numpy as np
import pytest
import torch

from _reward_normalization import CASES, EPSILON, GAMMA, HOST_ERROR, STEPS, errors, inputs, make_hook, restate, run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


@pytest.fixture(scope="module")
def references():
    """Per case: the inputs, the float64 restatement and the host restatement's result, computed once."""
    from cusrl_amd import ops

    out = {}
    for case in CASES:
        data = inputs(*case)
        out[case] = dict(inputs=data, float64=restate(*data), host=run(ops.reward_normalize_cpu_, "cpu", *data))
    return out


def _assert_against_both(label, result, float64, host):
    figures = errors(result, float64)  # (the returns: the restatement's bits, asserted inside)
    apart = max(float((a[key].double() - b[key].double()).abs().max()) for a, b in zip(result, host) for key in ("stats", "reward"))
    print(f"{label}: kernel vs float64, stats {figures['stats']:.3e} (asserted {4 * HOST_ERROR['stats']:.1e}), reward "
          f"{figures['reward']:.3e} (asserted {4 * HOST_ERROR['reward']:.1e}); largest |kernel - host restatement| {apart:.3e}")
    for a, b in zip(result, host):
        assert torch.equal(a["returns"], b["returns"]), label
        assert torch.equal(a["stats"][2], b["stats"][2]), label
    for key, figure in figures.items():
        assert figure <= 4 * HOST_ERROR[key], (label, key, figure)


@pytest.mark.parametrize("case", CASES, ids=lambda case: f"N{case[0]}-R{case[1]}")
def test_kernel_against_float64_and_the_host_restatement(cusrl, references, case):
    from cusrl_amd import ops

    reference = references[case]
    reward, terminated, truncated = reference["inputs"]
    result = run(ops.reward_normalize_, DEV, reward, terminated, truncated)
    _assert_against_both(f"N = {case[0]}, R = {case[1]}", result, reference["float64"], reference["host"])
    for t, step in enumerate(result):
        done = torch.from_numpy(terminated[t] | truncated[t])
        assert (step["returns"][done] == 0).all() and (step["returns"][~done] != 0).all()


@pytest.mark.parametrize("case", [(1025, 1), (257, 2)], ids=lambda case: f"N{case[0]}-R{case[1]}")
def test_clamp_and_frozen_statistics_have_the_host_forms_bits(cusrl, references, case):
    from cusrl_amd import ops

    reward, terminated, truncated = references[case]["inputs"]
    for kwargs in (dict(clip=0.5), dict(clip=0.5, update=False), dict(update=False)):
        result = run(ops.reward_normalize_, DEV, reward, terminated, truncated, **kwargs)
        host = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated, **kwargs)
        _assert_against_both(f"{case} {kwargs}", result, restate(reward, terminated, truncated, **kwargs), host)
        for a, b in zip(result, host):
            if "clip" in kwargs:
                saturated = b["reward"].abs() == 0.5
                assert saturated.any() and torch.equal(a["reward"][saturated], b["reward"][saturated])
            if not kwargs.get("update", True):
                assert a["stats"].tolist() == [[0.0] * case[1], [1.0] * case[1], [1e-4] * case[1]]
                assert torch.equal(a["reward"], b["reward"])  # the scale is 1 or, clamped, the host form's


def _padded(rows: torch.Tensor, canary, pad=3, shift=0):
    N, width = rows.shape
    flat = torch.full(((N + 2 * pad) * width + shift,), canary, dtype=rows.dtype, device=DEV)
    buffer = flat[shift:].view(N + 2 * pad, width)
    buffer[pad : pad + N] = rows.to(DEV)
    return buffer, flat


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", [(1025, 1), (4099, 1), (257, 2)], ids=lambda case: f"N{case[0]}-R{case[1]}")
def test_a_launch_stays_inside_its_rows_and_alignment_changes_no_bit(cusrl, references, case, offset):
    """The C entry on over-allocated buffers, canary rows before and after every operand; ``offset = 1``: the reward starts one
    float off the 16-byte boundary, so with R = 1 the chunks move as scalars — the same bits as the vector accesses.  Two steps from
    a state the op produced; the second repeated from a copy of the same state gives the same bits again."""
    from cusrl_amd import _native, ops

    N, R = case
    reward, terminated, truncated = references[case]["inputs"]
    first = run(ops.reward_normalize_, DEV, reward[:2], terminated[:2], truncated[:2], clip=3.0)
    pad = 4  # (a multiple of 4 rows keeps the inner rows of the R = 1 operands on their 16-byte boundary at offset 0)
    canaries = {"reward": 7.5, "G": -3.25, "terminated": 77, "truncated": 78}
    stats = torch.full((5, R), 12345.0, dtype=torch.float64, device=DEV)
    stats[1:4] = torch.tensor([[0.0] * R, [1.0] * R, [1e-4] * R], dtype=torch.float64)
    outputs = []
    for t in range(2):
        rows = {"reward": torch.from_numpy(reward[t]), "G": first[t - 1]["returns"] if t else torch.zeros(N, R),
                "terminated": torch.from_numpy(terminated[t]).view(N, 1).to(torch.uint8),
                "truncated": torch.from_numpy(truncated[t]).view(N, 1).to(torch.uint8)}
        for repeat in range(2 if t else 1):
            buffers = {key: _padded(value, canaries[key], pad, offset if key == "reward" else 0) for key, value in rows.items()}
            before = {key: value[0].clone() for key, value in buffers.items()}
            inner = {key: value[0][pad:].data_ptr() for key, value in buffers.items()}
            assert inner["reward"] % 16 == (4 * offset if R == 1 else inner["reward"] % 16) and inner["G"] % 4 == 0
            state = stats.clone()
            status = _native.lib().cusrl_reward_normalize(inner["reward"], inner["G"], inner["terminated"], inner["truncated"],
                                                          state[1:].data_ptr(), GAMMA, EPSILON, 3.0, 1, 1, N, R,
                                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert status == 0
            torch.cuda.synchronize()
            for key, (buffer, flat) in buffers.items():
                assert torch.equal(buffer[:pad], before[key][:pad]) and torch.equal(buffer[pad + N :], before[key][pad + N :]), key
                assert (flat[: flat.numel() - buffer.numel()] == canaries[key]).all()
            for key in ("terminated", "truncated"):
                assert torch.equal(buffers[key][0], before[key])
            assert (state[0] == 12345.0).all() and (state[4] == 12345.0).all()
            outputs.append((buffers["reward"][0][pad : pad + N].cpu(), buffers["G"][0][pad : pad + N].cpu(), state[1:4].cpu()))
        stats = state
        assert torch.equal(outputs[-1][0], first[t]["reward"]) and torch.equal(outputs[-1][1], first[t]["returns"])
        assert torch.equal(outputs[-1][2], first[t]["stats"])
    for a, b in zip(outputs[1], outputs[2]):  # the same state twice: identical bits
        assert torch.equal(a, b)


def test_launch_census(cusrl):
    """One ``post_step`` is exactly one ``cusrl_reward_normalize``, by the call counter and by the node list of a graph captured
    around it (one kernel node, no memset, no copy)."""
    from cusrl_amd import _native, ops

    reward, terminated, truncated = inputs(257, 1)
    hook = make_hook(cusrl, 257, 1, DEV, clip=10.0)
    transition = {"reward": torch.from_numpy(reward[0].copy()).to(DEV), "terminated": torch.from_numpy(terminated[0]).to(DEV).unsqueeze(-1),
                  "truncated": torch.from_numpy(truncated[0]).to(DEV).unsqueeze(-1)}
    before = dict(_native.launch_counts)
    hook.post_step(transition)
    moved = {key: value - before.get(key, 0) for key, value in _native.launch_counts.items() if value != before.get(key, 0)}
    assert moved == {"cusrl_reward_normalize": 1}, moved
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=stream):
        hook.post_step(transition)
    census = ops.graph_census(graph)
    assert (census["kernel"], census["memcpy"], census["memset"], census["other"]) == (1, 0, 0, 0), census
    assert "reward_normalize_kernel" in census["names"][0], census["names"]
    torch.cuda.synchronize()


def test_c_entry_refusals(cusrl):
    """Return codes only, nothing invalid is launched (device pointers; the host-side table: tests/test_reward_normalization.py)."""
    from cusrl_amd import _native

    lib = _native.lib()
    reward, G = torch.ones(9, 1, device=DEV), torch.zeros(9, 1, device=DEV)
    flags = torch.zeros(9, dtype=torch.uint8, device=DEV)
    stats = torch.tensor([[0.0], [1.0], [1e-4]], dtype=torch.float64, device=DEV)

    def call(**kw):
        P = lambda name, tensor: kw[name] if name in kw else tensor.data_ptr()  # noqa: E731
        return lib.cusrl_reward_normalize(P("reward", reward), P("G", G), P("terminated", flags), P("truncated", flags), P("stats", stats),
                                          GAMMA, EPSILON, kw.get("clip", 0.0), kw.get("has_clip", 0), 1, kw.get("N", 8), kw.get("R", 1), None)

    assert call(N=-1) == -1 and call(R=0) == -1 and call(stats=None) == -1 and call(reward=None) == -1 and call(truncated=None) == -1
    assert call(reward=reward.data_ptr() + 2) == -1 and call(stats=stats.data_ptr() + 4) == -1
    assert call(has_clip=1, clip=-1.0) == -1 and call(R=65536) == -3 and call(N=2**62, R=2) == -3 and call(N=0) == 0
    torch.cuda.synchronize()
    assert (reward == 1).all() and not G.any() and stats.tolist() == [[0.0], [1.0], [1e-4]]
    assert call(reward=reward[1:].data_ptr()) == 0  # one float off the 16-byte boundary: taken, as scalars
    torch.cuda.synchronize()
    assert reward[0] == 1 and stats[2, 0] == 8.0001


# ------------------------------------------------------------------------------------------------ inside the trainer
def _trainer(cusrl, seed, iterations, compile=True, extra_hooks=(), **trainer_kwargs):
    cusrl.set_global_seed(seed)
    env = cusrl.environment.make("Pendulum", 8, device=DEV, max_episode_steps=16)
    factory = cusrl.preset.PpoAgentFactory(
        num_steps_per_update=12, sampler_epochs=2, sampler_mini_batches=2, compile=compile, actor_hidden_dims=(64, 64),
        critic_hidden_dims=(64, 64), activation_fn="Tanh", optimizer_kwargs={"capturable": True, "fused": True}).to_underlying()
    for hook in extra_hooks:
        factory.register_hook(hook, before="value_computation")
    factory.register_hook(cusrl.hook.RewardNormalization(clip=10.0), before="value_computation")
    return cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False, **trainer_kwargs)


def _assert_same_run(a, b):
    assert set(a.agent.buffer.storage) == set(b.agent.buffer.storage)
    for key in a.agent.buffer.storage:
        assert torch.equal(a.agent.buffer.storage[key], b.agent.buffer.storage[key]), key
    for (name, p), q in zip(a.agent.named_parameters(), b.agent.parameters()):
        assert torch.equal(p, q), name
    for name in ("returns", "stats"):
        assert torch.equal(getattr(a.agent.hook["reward_normalization"].statistics, name),
                           getattr(b.agent.hook["reward_normalization"].statistics, name)), name
    for attr in ("state", "steps", "episode"):
        assert torch.equal(getattr(a.environment, attr), getattr(b.environment, attr)), attr


def test_captured_rollout_is_bit_identical_to_the_host_driven_loop(cusrl):
    """Pendulum, 8 envs, 16-step episodes, 12-step rollouts, 4 iterations from the same seed with the hook registered, host-driven
    against ``compile=True`` capture: every buffer leaf, every parameter, the hook's state, the episode statistics and the env."""
    runs = []
    for capture in (False, True):
        trainer = _trainer(cusrl, 21, 4)
        trainer.capture_rollout = capture
        trainer.run_training_loop()
        runs.append(trainer)
    host, captured = runs
    assert host._graphed_rollout is None
    graphed = captured._graphed_rollout
    assert graphed is not None and graphed.captured == 12 and len(graphed.rollouts) == 1, (graphed and graphed.captured)
    _assert_same_run(host, captured)
    for attr in ("episode_rew", "episode_len", "rew_buffer", "len_buffer"):
        assert torch.equal(getattr(host.stats, attr), getattr(captured.stats, attr)), attr
    assert host.stats.num_episodes == captured.stats.num_episodes and host.stats.num_episodes > 0
    statistics = host.agent.hook["reward_normalization"].statistics
    assert statistics.count[0].item() == 1e-4 + 4 * 12 * 8 and torch.isfinite(statistics.stats).all()
    assert (host.agent.buffer["reward"].abs() <= 10.0).all() and host.agent.buffer["truncated"].any()


def test_buffer_holds_the_normalised_reward_and_the_log_the_raw_one(cusrl):
    """Two host-driven iterations with a spy in front of the hook: the buffer holds what the host restatement makes of the raw
    rewards within the kernel bound, the trainer's episode returns are sums of the raw ones."""
    from cusrl_amd import ops

    class Spy(cusrl.Hook):
        seen = []

        def post_step(self, transition):
            self.seen.append(tuple(transition[key].cpu().clone() for key in ("reward", "terminated", "truncated")))

    trainer = _trainer(cusrl, 3, 2, compile=False, extra_hooks=[Spy()])
    trainer.run_training_loop()
    hook = trainer.agent.hook["reward_normalization"]
    assert len(Spy.seen) == 24 and hook.statistics.count[0].item() == 1e-4 + 24 * 8
    G, stats = torch.zeros(8, 1), torch.tensor([[0.0], [1.0], [1e-4]], dtype=torch.float64)
    running, episodes = torch.zeros(8), []
    for t, (raw, terminated, truncated) in enumerate(Spy.seen):
        running += raw[:, 0]
        done = (terminated | truncated)[:, 0]
        episodes += running[done].tolist()
        running[done] = 0
        scaled = ops.reward_normalize_cpu_(raw.clone(), G, terminated, truncated, stats, 0.99, 1e-8, 10.0)
        assert not torch.equal(scaled, raw)
        if t >= 12:
            stored = trainer.agent.buffer["reward"][t - 12].cpu()
            assert float(((stored - scaled).abs() / scaled.abs().clamp(min=1.0)).max()) <= 4 * HOST_ERROR["reward"]
    assert torch.equal(hook.statistics.returns.cpu(), G)
    assert float(((hook.statistics.stats.cpu() - stats).abs() / stats.abs().clamp(min=1.0)).max()) <= 4 * HOST_ERROR["stats"]
    count = trainer.stats.num_episodes
    assert count == len(episodes) > 0
    np.testing.assert_allclose(sorted(trainer.stats.rew_buffer[:count, 0].tolist()), sorted(episodes), rtol=1e-5)


def test_checkpoint_round_trip_continues_bit_identically(cusrl, tmp_path):
    """Saved after 2 iterations and loaded into a fresh trainer (other seed, so everything it continues from is the checkpoint's):
    the next iteration equals the one the first trainer goes on with, and the hook's state was loaded in place."""
    first = _trainer(cusrl, 21, 2, compile=False)
    first.run_training_loop()
    path = tmp_path / "ckpt_2.pt"
    torch.save({"agent": first.agent.state_dict(), "environment": first.environment.state_dict(), "iteration": first.iteration,
                "stats": first.stats.state_dict()}, path)
    first.num_iterations = 3
    cusrl.set_global_seed(99)
    first.run_training_loop()
    fresh = _trainer(cusrl, 5, 3, compile=False)
    statistics = fresh.agent.hook["reward_normalization"].statistics
    addresses = statistics.returns.data_ptr(), statistics.stats.data_ptr()
    second = _trainer(cusrl, 5, 3, compile=False, checkpoint_path=str(path))
    statistics = second.agent.hook["reward_normalization"].statistics
    assert second.iteration == 2 and statistics.count[0].item() == 1e-4 + 2 * 12 * 8 and statistics.returns.any()
    fresh.agent.load_state_dict(torch.load(path, map_location=DEV)["agent"])  # ... in place, on a hook that already has its state
    assert (fresh.agent.hook["reward_normalization"].statistics.returns.data_ptr(),
            fresh.agent.hook["reward_normalization"].statistics.stats.data_ptr()) == addresses
    assert torch.equal(fresh.agent.hook["reward_normalization"].statistics.stats, statistics.stats)
    cusrl.set_global_seed(99)
    second.run_training_loop()
    assert first.iteration == second.iteration == 3
    _assert_same_run(first, second)
    assert statistics.count[0].item() == 1e-4 + 3 * 12 * 8
