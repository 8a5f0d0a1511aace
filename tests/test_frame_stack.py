"""Frame stacking in its host form (no GPU): the library's host restatements of the two kernels (``cusrl_frame_stack_push_cpu`` /
``cusrl_frame_stack_reset_cpu``) against the numpy restatement of gymnasium's ``FrameStackObservation`` (tests/_frame_stack.py
``DequeStack``), bit for bit; the stale-entry and fresh-flag contracts; ``nn.ObservationStacker`` and ``environment.FrameStack`` over
a scripted env; the argument errors; the C ABI.  The kernels: tests/test_frame_stack_gpu.py."""

import numpy as np
import pytest
import torch

from _frame_stack import (
    SCRIPT_ENVS, SCRIPT_RESETS, SCRIPT_STEPS, SPECIAL_WORDS, DequeStack, ScriptedEnvironment, expected, frames, words,
)

COLUMN_CASES = {1: (None, [0]), 3: (None, [2, 0], [1, 2, 0]), 4: (None, [3, 1], [2, 0, 3, 1])}


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def test_the_inputs_hold_every_special_word():
    data = frames(3, SCRIPT_STEPS, SCRIPT_ENVS, 4).view(np.uint32)
    assert all((data == word).any() for word in SPECIAL_WORDS)
    assert np.isnan(frames(3, 6).view(np.float32)).sum() == 2


@pytest.mark.parametrize("padding", ["reset", "zero"])
@pytest.mark.parametrize("K0", [1, 3, 4])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_host_restatements_against_the_deque(cusrl, S, K0, padding):
    """3 envs, 6 steps, env 0 reset after step 0, env 1 after steps 2 and 3, env 2 never; without ``columns``, with a subset and with
    a permutation; frames holding NaNs with payloads, -0.0, +-Inf and a denormal.  After every call ``out`` and ``H`` hold the
    deque's bits and ``out`` is a buffer of its own."""
    from cusrl_amd import ops

    for columns in COLUMN_CASES[K0]:
        N, K = SCRIPT_ENVS, K0 if columns is None else len(columns)
        table, reset_table = frames(10 * S + K0, SCRIPT_STEPS, N, K0), frames(10 * S + K0 + 1, SCRIPT_STEPS, N, K0)
        table_t, reset_t = torch.from_numpy(table), torch.from_numpy(reset_table)
        column_table = ops.frame_stack_columns(columns, K0, "cpu")
        reference = DequeStack(N, S, padding, columns)
        H = torch.full((N, S, K), 7.0)

        def check(out, label):
            assert torch.equal(words(H).view(N, -1), expected(reference.rows())), label
            assert out.untyped_storage().data_ptr() != H.untyped_storage().data_ptr()

        out = ops.frame_stack_reset_cpu(H, torch.arange(N), None, reset_t[0], column_table, padding)
        for env in range(N):
            reference.reset(env, reset_table[0, env])
        assert tuple(out.shape) == (N, S * K) and torch.equal(words(out), expected(reference.rows()))
        check(out, (columns, "first reset"))
        resets = 1
        for t in range(SCRIPT_STEPS):
            out = ops.frame_stack_push_cpu(H, table_t[t], column_table, None, padding)
            for env in range(N):
                reference.step(env, table[t, env])
            assert tuple(out.shape) == (N, S * K) and torch.equal(words(out), expected(reference.rows())), (columns, t)
            check(out, (columns, t))
            ids = SCRIPT_RESETS.get(t)
            if ids:
                out = ops.frame_stack_reset_cpu(H, torch.tensor(ids), None, reset_t[resets][ids], column_table, padding)
                for j, env in enumerate(ids):
                    reference.reset(env, reset_table[resets, env])
                    assert torch.equal(words(out[j]), expected(reference.row(env))), (columns, t, env)
                check(out, (columns, t, "reset"))
                resets += 1
        assert resets == 4


@pytest.mark.parametrize("padding", ["reset", "zero"])
@pytest.mark.parametrize("count", [0, 2, 5, None])
def test_stale_entries_never_write_the_history(cusrl, count, padding):
    """``L = 5`` slots over 6 envs: ``H`` changes for the first ``count`` ids only, their ``out`` rows are the refilled histories,
    a stale slot's row is its env's history — also where a stale id (the last slot's 3) repeats a valid one (slot 0)."""
    from cusrl_amd import ops

    N, S, K, L = 6, 3, 2, 5
    live = L if count is None else count
    ids = [3, 1, 0, 4, 2] if live == L else [3, 1, 0, 4, 3]  # (the valid ids are distinct)
    H = torch.from_numpy(frames(1, N, S, K).copy())
    before = H.clone()
    rows = frames(2, L, K)
    reference = DequeStack(N, S, padding)
    out = ops.frame_stack_reset_cpu(H, torch.tensor(ids), None if count is None else torch.tensor([count], dtype=torch.int32),
                                    torch.from_numpy(rows), None, padding)
    for j in range(live):
        reference.reset(ids[j], rows[j])
        assert torch.equal(words(out[j]), expected(reference.row(ids[j]))), j
        assert torch.equal(words(H[ids[j]]).view(-1), expected(reference.row(ids[j]))), j
    untouched = [env for env in range(N) if env not in ids[:live]]
    assert torch.equal(words(H[untouched]), words(before[untouched]))
    for j in range(live, L):
        assert torch.equal(words(out[j]), words(H[ids[j]]).view(-1)), j  # (the host form walks the slots in order: the new history)


@pytest.mark.parametrize("padding", ["reset", "zero"])
def test_fresh_rows_are_refilled_and_their_flags_cleared(cusrl, padding):
    """A flagged row of a push is what the reset entry makes of the same observation; the other rows are shifted; only the flags
    that were set are cleared."""
    from cusrl_amd import ops

    N, S, K = 5, 4, 3
    start, obs = frames(4, N, S, K), frames(5, N, K)
    flagged = [0, 3]
    fresh = torch.zeros(N, dtype=torch.bool)
    fresh[flagged] = True
    H = torch.from_numpy(start.copy())
    out = ops.frame_stack_push_cpu(H, torch.from_numpy(obs), None, fresh, padding)
    assert not fresh.any()
    by_reset = torch.from_numpy(start.copy())
    rows = ops.frame_stack_reset_cpu(by_reset, torch.tensor(flagged), None, torch.from_numpy(obs[flagged]), None, padding)
    assert torch.equal(words(out[flagged]), words(rows)) and torch.equal(words(H[flagged]), words(by_reset[flagged]))
    others = [1, 2, 4]
    shifted = np.concatenate([start[others, 1:], obs[others, None]], axis=1)
    assert torch.equal(words(H[others]), words(torch.from_numpy(shifted))) and torch.equal(words(out), words(H).view(N, -1))
    # uint8 flags, and none of them set: every row shifts
    flags = torch.zeros(N, dtype=torch.uint8)
    again = ops.frame_stack_push_cpu(H, torch.from_numpy(obs), None, flags, padding)
    assert torch.equal(words(again[:, -K:]), words(torch.from_numpy(obs))) and torch.equal(words(again[:, :K]), words(out[:, K:2 * K]))


@pytest.mark.parametrize("padding", ["reset", "zero"])
@pytest.mark.parametrize("columns", [None, [2, 0]])
def test_observation_stacker_on_the_host(cusrl, columns, padding):
    N, K0, S = SCRIPT_ENVS, 3, 4
    K = K0 if columns is None else len(columns)
    stacker = cusrl.nn.ObservationStacker(K0, S, padding, columns)
    assert stacker is not None and cusrl.ObservationStacker is cusrl.nn.ObservationStacker
    assert stacker.output_dim == S * K and stacker.history is None
    table = frames(6, SCRIPT_STEPS + 1, N, K0)
    reference = DequeStack(N, S, padding, columns)
    pending = set(range(N))  # the rows whose next observation starts a history
    for t in range(SCRIPT_STEPS + 1):
        done = torch.zeros(N, 1, dtype=torch.bool)
        done[SCRIPT_RESETS.get(t, [])] = True
        if t % 2:  # a call with done= is a call followed by reset(done)
            out = stacker(torch.from_numpy(table[t]), done=done)
        else:
            out = stacker(torch.from_numpy(table[t]))
            stacker.reset(done.squeeze(-1))
        for env in range(N):
            (reference.reset if env in pending else reference.step)(env, table[t, env])
        pending = set(SCRIPT_RESETS.get(t, []))
        assert tuple(out.shape) == (N, S * K) and torch.equal(words(out), expected(reference.rows())), t
        assert torch.equal(words(stacker.history).view(N, -1), words(out))
        assert out.untyped_storage().data_ptr() != stacker.history.untyped_storage().data_ptr()
    stacker.reset()
    out = stacker(torch.from_numpy(table[0]))
    for env in range(N):
        reference.reset(env, table[0, env])
    assert torch.equal(words(out), expected(reference.rows()))
    # another batch size is refused with DeployedPolicy's remedy; history = None starts over
    with pytest.raises(ValueError, match=r"holds 3 rows, the observation 2; assign 'history = None' to start over with another batch size"):
        stacker(torch.zeros(2, K0))
    stacker.history = None
    assert stacker(torch.ones(2, K0)).shape == (2, S * K)
    with pytest.raises(ValueError, match=r"\[B, 3\]"):
        stacker(torch.zeros(2, K0 + 1))
    with pytest.raises(TypeError, match="bool"):
        stacker(torch.zeros(2, K0), done=torch.zeros(2))
    # other dtypes are evaluated in fp32
    assert stacker(torch.ones(2, K0, dtype=torch.float64)).dtype == torch.float32


def _scripted(**properties):
    table, reset_table = frames(7, SCRIPT_STEPS, SCRIPT_ENVS, 3), frames(8, SCRIPT_STEPS, SCRIPT_ENVS, 3)
    return ScriptedEnvironment(table, reset_table, SCRIPT_RESETS, **properties), table, reset_table


@pytest.mark.parametrize("padding", ["reset", "zero"])
@pytest.mark.parametrize("columns", [None, [2, 0]])
def test_frame_stack_wrapper_on_the_host(cusrl, columns, padding):
    """The wrapper driven as the trainer drives an env — step, then ``reset(indices=...)`` of the finished envs — over a scripted
    env: widths, passthrough of state, reward, flags and info, the terminal observation in a finished env's stacked row."""
    inner, table, reset_table = _scripted(action_denormalization=(1.0, 2.0), custom_extra="kept")
    twin, _, _ = _scripted()
    N, K0, S = SCRIPT_ENVS, 3, 4
    K = K0 if columns is None else len(columns)
    env = cusrl.environment.FrameStack(inner, S, padding, columns)
    assert isinstance(env, cusrl.Environment) and cusrl.FrameStack is cusrl.environment.FrameStack
    assert (env.observation_dim, env.spec.observation_dim, env.action_dim, env.num_instances) == (S * K, S * K, 2, N)
    assert (env.spec.state_dim, env.spec.reward_dim, env.spec.timestep, env.spec.autoreset) == (2, 1, 0.02, False)
    assert env.spec.action_denormalization == (1.0, 2.0) and env.spec.custom_extra == "kept"
    assert env.spec.environment_instance is env and env.spec.num_instances == N
    assert not env.capturable and not env.generator_free
    reference = DequeStack(N, S, padding, columns)
    observation, state, info = env.reset(randomize_episode_progress=True)
    twin_observation, twin_state, twin_info = twin.reset()
    for e in range(N):
        reference.reset(e, reset_table[0, e])
    assert torch.equal(words(observation), expected(reference.rows())) and torch.equal(state, twin_state) and info == twin_info
    resets = 0
    for t in range(SCRIPT_STEPS):
        action = torch.zeros(N, 2)
        stepped, expected_step = env.step(action), twin.step(action)
        for e in range(N):
            reference.step(e, table[t, e])
        # the newest slot of EVERY row is the inner step's observation: for a finished env its terminal observation
        assert torch.equal(words(stepped[0]), expected(reference.rows())), t
        assert torch.equal(words(stepped[0][:, -K:]), words(expected_step[0] if columns is None else expected_step[0][:, columns]))
        for got, want in zip(stepped[1:5], expected_step[1:5]):
            assert got.dtype == want.dtype and torch.equal(got, want), t
        assert stepped[5] == expected_step[5]
        ids = SCRIPT_RESETS.get(t)
        if ids:
            resets += 1
            rows, state, info = env.reset(indices=ids)
            _, twin_state, twin_info = twin.reset(indices=ids)
            for j, e in enumerate(ids):
                reference.reset(e, reset_table[resets, e])
                assert torch.equal(words(rows[j]), expected(reference.row(e))), (t, e)
            assert torch.equal(state, twin_state) and info == twin_info
            assert torch.equal(words(env.history).view(N, -1), expected(reference.rows()))
    assert env.get_metrics() == {"scripted": 1.0} and env.state_dict() == {"t": SCRIPT_STEPS}
    env.close()
    assert inner.closed


def test_frame_stack_refuses_what_it_cannot_translate(cusrl):
    FrameStack = cusrl.environment.FrameStack
    for name, value in (("observation_stat_groups", ((0, 2),)), ("mirror_observation", object()),
                        ("observation_normalization", (torch.zeros(3), torch.ones(3))),
                        ("observation_normalization_excluded_indices", [1]), ("observation_is_subset_of_state", [0, 1, 2])):
        inner, _, _ = _scripted(**{name: value})
        with pytest.raises(ValueError, match=name):
            FrameStack(inner, 2)
    inner, _, _ = _scripted(autoreset=True)
    with pytest.raises(ValueError, match="autoreset"):
        FrameStack(inner, 2)
    inner, _, _ = _scripted()
    with pytest.raises(ValueError, match="stack_size must be at least 1"):
        FrameStack(inner, 0)
    with pytest.raises(ValueError, match="padding_type"):
        FrameStack(inner, 2, "edge")
    with pytest.raises(ValueError, match="distinct"):
        FrameStack(inner, 2, columns=[1, 1])
    with pytest.raises(TypeError, match="Environment"):
        FrameStack(object(), 2)


def test_make_wraps_on_request_only(cusrl):
    env = cusrl.environment
    bare = env.make("CartPole", 4, device="cpu", seed=3)
    assert type(bare) is env.CartPole
    stacked = env.make("CartPole", 4, device="cpu", seed=3, frame_stack=3)
    assert type(stacked) is env.FrameStack and type(stacked.env) is env.CartPole and stacked.observation_dim == 12
    assert stacked.spec.reward_dim == 1 and stacked.stack_size == 3 and stacked.padding_type == "reset"
    observation, state, info = stacked.reset()
    assert torch.equal(observation, bare.reset()[0].repeat(1, 3)) and state is None and info == {}
    positions = env.FrameStack(env.make("CartPole", 4, device="cpu", seed=3), 4, columns=[0, 2])
    first = env.make("CartPole", 4, device="cpu", seed=3).reset()[0]
    assert positions.observation_dim == 8 and torch.equal(positions.reset()[0], first[:, [0, 2]].repeat(1, 4))
    with pytest.raises(ValueError, match="CartPole, Pendulum, MountainCar"):
        env.make("Acrobot", 4, frame_stack=2)


def test_argument_checks(cusrl):
    from cusrl_amd import _native, ops

    H, obs = torch.zeros(3, 2, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match=r"'H' must be a contiguous fp32 \[N, S, K\] CPU tensor; got torch.float64"):
        ops.frame_stack_push_cpu(H.double(), obs)
    with pytest.raises(ValueError, match=r"'H'.*strided"):
        ops.frame_stack_push_cpu(torch.zeros(3, 4, 2).transpose(1, 2), obs)
    with pytest.raises(ValueError, match=r"'obs' must be a contiguous fp32 \[3, K0\].*torch.float16"):
        ops.frame_stack_push_cpu(H, obs.half())
    with pytest.raises(ValueError, match=r"'obs'.*strided"):
        ops.frame_stack_push_cpu(H, torch.zeros(4, 3).t())
    with pytest.raises(ValueError, match="'H' is 4 wide and the observation 5"):
        ops.frame_stack_push_cpu(H, torch.zeros(3, 5))
    with pytest.raises(ValueError, match=r"'columns' must be a contiguous int32 \[4\]"):
        ops.frame_stack_push_cpu(H, torch.zeros(3, 5), torch.tensor([0, 1, 2, 3]))
    with pytest.raises(ValueError, match=r"'columns' must index a 5-wide observation"):
        ops.frame_stack_push_cpu(H, torch.zeros(3, 5), torch.tensor([0, 1, 2, 5], dtype=torch.int32))
    with pytest.raises(ValueError, match="'columns' must be distinct"):
        ops.frame_stack_push_cpu(H, torch.zeros(3, 5), torch.tensor([0, 1, 2, 1], dtype=torch.int32))
    for bad, message in (([0, 7], "index a 5-wide"), ([-1], "index a 5-wide"), ([2, 2], "distinct"), ([], "non-empty"), ([0.5], "ints")):
        with pytest.raises(ValueError, match=message):
            ops.frame_stack_columns(bad, 5, "cpu")
    assert ops.frame_stack_columns(None, 5, "cpu") is None
    with pytest.raises(ValueError, match="'fresh' must be a contiguous bool tensor of 3 flags"):
        ops.frame_stack_push_cpu(H, obs, None, torch.zeros(2, dtype=torch.bool))
    with pytest.raises(ValueError, match="padding_type must be one of"):
        ops.frame_stack_push_cpu(H, obs, None, None, "edge")
    with pytest.raises(ValueError, match="overlaps 'H'"):
        ops.frame_stack_push_cpu(H, obs, out=H.view(3, 8))
    with pytest.raises(ValueError, match="stack_size >= 1"):
        ops.frame_stack_push_cpu(torch.zeros(3, 0, 4), obs)
    with pytest.raises(ValueError, match="'indices' must be a contiguous int64"):
        ops.frame_stack_reset_cpu(H, torch.zeros(2, dtype=torch.int32), None, obs[:2])
    with pytest.raises(ValueError, match="'count' must be a 1-element int32"):
        ops.frame_stack_reset_cpu(H, torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), obs[:2])
    with pytest.raises(ValueError, match=r"'reset_obs' must be a contiguous fp32 \[2, K0\]"):
        ops.frame_stack_reset_cpu(H, torch.zeros(2, dtype=torch.int64), None, obs)
    with pytest.raises(ValueError, match="device tensor; got torch.float32"):
        ops.frame_stack_push(H, obs)  # the device entry has no host form behind it
    assert not ops.frame_stack_supported(H, obs)
    with pytest.raises(ValueError, match="stack_size must be at least 1"):
        cusrl.nn.ObservationStacker(4, 0)
    with pytest.raises(ValueError, match="distinct"):
        cusrl.nn.ObservationStacker(4, 2, columns=[0, 0])
    # an id outside [0, N) is skipped: no history is touched, its row is zeros; empty calls do nothing
    H.fill_(0.5)
    rows = ops.frame_stack_reset_cpu(H, torch.tensor([7, -1, 1]), None, torch.ones(3, 4))
    assert (rows[:2] == 0).all() and (rows[2] == 1).all() and (H[[0, 2]] == 0.5).all() and (H[1] == 1).all()
    assert ops.frame_stack_push_cpu(torch.zeros(0, 2, 4), torch.zeros(0, 4)).shape == (0, 8)
    assert ops.frame_stack_reset_cpu(H, torch.zeros(0, dtype=torch.int64), None, torch.zeros(0, 4)).shape == (0, 8)
    # the C entries: invalid pointers, pairs and extents are -1, overflow is -3, nothing is launched
    lib, p = _native.lib(), 0x1000
    assert lib.cusrl_frame_stack_push(None, p + 0x100, None, None, p + 0x200, 4, 2, 4, 4, 0, None) == -1
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 0x200, 4, 2, 4, 5, 0, None) == -1  # K != K0 without columns
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 0x200, 4, 0, 4, 4, 0, None) == -1  # S < 1
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 0x200, 4, 2, 4, 4, 2, None) == -1  # padding code
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 2, 4, 2, 4, 4, 0, None) == -1      # misaligned
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 64, 4, 2, 4, 4, 0, None) == -1     # out overlaps H
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 0x200, 4, 2, 2**31, 2**31, 0, None) == -3
    assert lib.cusrl_frame_stack_push(p, p + 0x100, None, None, p + 0x200, 2**40, 2**20, 4, 4, 0, None) == -3
    assert lib.cusrl_frame_stack_push(None, None, None, None, None, 0, 2, 4, 4, 0, None) == 0
    assert lib.cusrl_frame_stack_reset(p, None, None, p + 0x100, None, p + 0x200, 2, 4, 2, 4, 4, 0, None) == -1
    assert lib.cusrl_frame_stack_reset(p, p + 0x300, None, p + 0x100, None, p + 0x200, -1, 4, 2, 4, 4, 0, None) == -1
    assert lib.cusrl_frame_stack_reset(p, p + 0x300, None, p + 0x100, None, p + 0x200, 2, 4, 2, 4, 2**31, 1, None) == -1
    assert lib.cusrl_frame_stack_reset(p, p + 0x300, None, p + 0x100, p + 0x400, p + 0x200, 2, 4, 2, 4, 2**31, 1, None) == -3
    assert lib.cusrl_frame_stack_reset(None, None, None, None, None, None, 0, 4, 2, 4, 4, 1, None) == 0


def test_abi_and_names(cusrl):
    import re
    from pathlib import Path

    from cusrl_amd import _native

    symbols = {"cusrl_frame_stack_push", "cusrl_frame_stack_push_cpu", "cusrl_frame_stack_reset", "cusrl_frame_stack_reset_cpu"}
    header = (Path(__file__).resolve().parent.parent / "include" / "cusrl_hip.h").read_text()
    assert symbols <= set(re.findall(r"\b(cusrl_[a-z0-9_]+)\s*\(", header))
    assert symbols <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert all(hasattr(_native.lib(), symbol) for symbol in symbols)
    assert (_native._CONSTANTS["FRAME_STACK_PAD_RESET"], _native._CONSTANTS["FRAME_STACK_PAD_ZERO"]) == (0, 1)
    assert "FrameStack" in cusrl.__all__ and "FrameStack" in cusrl.environment.__all__
    assert "ObservationStacker" in cusrl.__all__ and "ObservationStacker" in cusrl.nn.__all__
    from cusrl_amd import ops

    for name in ("frame_stack_push", "frame_stack_reset", "frame_stack_push_cpu", "frame_stack_reset_cpu", "frame_stack_supported"):
        assert callable(getattr(ops, name)) and name in ops.frame_stack.__all__
