"""``RewardNormalization`` without a GPU: the library's host restatement (``cusrl_reward_normalize_cpu``, the hook's host form)
against the float64 restatement of tests/_reward_normalization.py, the frozen, clamped, single-env and non-finite cases, the C
entry's refusals and the hook's own bookkeeping.  The kernel: tests/test_reward_normalization_gpu.py."""

import numpy as np
import pytest
import torch

import cusrl_amd as cusrl
from _reward_normalization import CASES, EPSILON, GAMMA, HOST_ERROR, STEPS, errors, inputs, make_hook, restate, run
from cusrl_amd import _native, ops


@pytest.fixture(scope="module")
def references():
    """Per case: the inputs and the float64 restatement, computed once."""
    return {case: (inputs(*case), restate(*inputs(*case))) for case in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda case: f"N{case[0]}-R{case[1]}")
def test_host_restatement_against_float64(references, case):
    """The running triple and the scaled reward after each of the 6 steps within 2 x the measured error, the returns to the bit
    (asserted inside ``errors``), finished envs' returns exactly 0."""
    (reward, terminated, truncated), expected = references[case]
    result = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated)
    figures = errors(result, expected)
    print(f"N = {case[0]}, R = {case[1]}: host restatement vs float64, stats {figures['stats']:.3e} (asserted "
          f"{2 * HOST_ERROR['stats']:.1e}), reward {figures['reward']:.3e} (asserted {2 * HOST_ERROR['reward']:.1e})")
    for t, step in enumerate(result):
        done = torch.from_numpy(terminated[t] | truncated[t])
        assert done[0] == (t in (0, 2, 3, 5)) and (step["returns"][done] == 0).all()
        assert (step["returns"][~done] != 0).all()
        assert step["stats"][2].tolist() == expected[t]["stats"][2].tolist()  # the count: the same additions
    for key, figure in figures.items():
        assert figure <= 2 * HOST_ERROR[key], (key, figure)


def test_measured_host_error_is_what_the_bounds_are_made_of(references):
    """``HOST_ERROR`` is the achieved figure over all cases rounded UP to two digits: never more than 10 % above what is measured."""
    worst = {"stats": 0.0, "reward": 0.0}
    for case, ((reward, terminated, truncated), expected) in references.items():
        for key, figure in errors(run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated), expected).items():
            worst[key] = max(worst[key], figure)
    print(f"worst over all cases: stats {worst['stats']:.3e}, reward {worst['reward']:.3e}")
    for key in worst:
        assert worst[key] <= HOST_ERROR[key] <= 1.1 * worst[key], (key, worst[key], HOST_ERROR[key])


def test_frozen_statistics_stay_bit_unchanged(references):
    (reward, terminated, truncated), _ = references[(257, 2)]
    result = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated, update=False)
    expected = restate(reward, terminated, truncated, update=False)
    for step in result:
        assert step["stats"].tolist() == [[0.0, 0.0], [1.0, 1.0], [1e-4, 1e-4]]
    figures = errors(result, expected)  # var = 1: the scale is sqrt(1 + 1e-8) rounded to fp32, which is 1
    assert figures["reward"] <= 2 * HOST_ERROR["reward"]
    assert np.array_equal(result[-1]["reward"].numpy(), reward[-1])


def test_clip_saturates_exactly(references):
    (reward, terminated, truncated), _ = references[(1025, 1)]
    clip = 0.5
    result = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated, clip=clip)
    expected = restate(reward, terminated, truncated, clip=clip)
    assert errors(result, expected)["reward"] <= 2 * HOST_ERROR["reward"]
    for got, want in zip(result, expected):
        saturated = np.abs(want["reward"]) == clip
        assert saturated.any() and not saturated.all()
        assert np.array_equal(got["reward"].numpy()[saturated], want["reward"][saturated].astype(np.float32))
        assert (got["reward"].abs() <= clip).all()


def test_a_single_env_has_batch_variance_zero_and_divides_by_no_zero(references):
    (reward, terminated, truncated), expected = references[(1, 1)]
    result = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated)
    first = result[0]["stats"][:, 0].tolist()
    G = float(reward[0, 0, 0])  # step 0: the return is the reward, merged with weight 1 / (1 + 1e-4) into (0, 1, 1e-4)
    assert first[2] == 1.0001 and abs(first[0] - G / 1.0001) <= 1e-15 * max(1.0, abs(G))
    assert abs(first[1] - (1e-4 + G * G * 1e-4 / 1.0001) / 1.0001) <= 1e-15 * max(1.0, G * G)
    for step in result:
        assert torch.isfinite(step["reward"]).all() and torch.isfinite(step["stats"]).all() and (step["stats"][1] > 0).all()


def test_a_nan_reward_propagates_and_the_call_returns():
    reward, terminated, truncated = inputs(257, 2)
    reward = reward.copy()
    reward[1, 5, 0] = np.nan  # step 1, env 5, column 0
    terminated[:, 5] = truncated[:, 5] = False
    result = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated)
    assert torch.isfinite(result[0]["reward"]).all() and torch.isfinite(result[0]["stats"]).all()
    for step in result[1:]:
        assert torch.isnan(step["returns"][5, 0]) and torch.isnan(step["stats"][:2, 0]).all()
        assert torch.isnan(step["reward"][:, 0]).all()  # the column's scale is a NaN from then on
        assert torch.isfinite(step["reward"][:, 1]).all() and torch.isfinite(step["stats"][:, 1]).all()
        assert torch.isfinite(step["returns"][:, 1]).all() and torch.isfinite(step["returns"][:5, 0]).all()
    inf = inputs(3, 1)[0].copy()
    inf[0, 1, 0] = np.inf
    result = run(ops.reward_normalize_cpu_, "cpu", inf, *inputs(3, 1)[1:])
    assert not torch.isfinite(result[0]["stats"][:2, 0]).any()


def test_c_entry_refusals_without_a_launch():
    """Return codes only (include/cusrl_hip.h): -1 invalid, -3 unsupported, 0 with nothing to do."""
    lib = _native.lib()
    assert {"cusrl_reward_normalize", "cusrl_reward_normalize_cpu"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    reward, G = torch.ones(8, 1), torch.zeros(8, 1)
    flags, stats = torch.zeros(8, dtype=torch.uint8), torch.tensor([[0.0], [1.0], [1e-4]], dtype=torch.float64)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(entry, **kw):
        args = [kw.get("reward", P(reward)), kw.get("G", P(G)), kw.get("terminated", P(flags)), kw.get("truncated", P(flags)),
                kw.get("stats", P(stats)), GAMMA, EPSILON, kw.get("clip", 0.0), kw.get("has_clip", 0), 1, kw.get("N", 8), kw.get("R", 1)]
        return entry(*args, None) if entry is lib.cusrl_reward_normalize else entry(*args)

    for entry in (lib.cusrl_reward_normalize, lib.cusrl_reward_normalize_cpu):
        assert call(entry, N=-1) == -1 and call(entry, R=0) == -1 and call(entry, R=-2) == -1
        for name in ("reward", "G", "terminated", "truncated", "stats"):
            assert call(entry, **{name: None}) == -1, name
        assert call(entry, reward=P(reward) + 2) == -1 and call(entry, G=P(G) + 1) == -1 and call(entry, stats=P(stats) + 4) == -1
        assert call(entry, has_clip=1, clip=-1.0) == -1 and call(entry, has_clip=1, clip=float("nan")) == -1
        assert call(entry, R=65536) == -3 and call(entry, N=2**62, R=2) == -3
        assert call(entry, N=0) == 0 and call(entry, N=0, reward=None, G=None, terminated=None, truncated=None, stats=None) == 0
    assert torch.equal(reward, torch.ones(8, 1)) and not G.any() and stats.tolist() == [[0.0], [1.0], [1e-4]]
    assert call(lib.cusrl_reward_normalize_cpu) == 0 and stats[2, 0] == 8.0001  # the same arguments, accepted


def test_the_op_checks_its_tensors():
    reward, G = torch.ones(8, 1), torch.zeros(8, 1)
    flags, stats = torch.zeros(8, 1, dtype=torch.bool), torch.tensor([[0.0], [1.0], [1e-4]], dtype=torch.float64)
    for bad in (dict(reward=reward.double()), dict(reward=torch.ones(8)), dict(returns=torch.zeros(4, 1)), dict(terminated=flags[:4]),
                dict(truncated=flags.float()), dict(stats=stats.float()), dict(stats=stats.t().contiguous()), dict(clip=-1.0),
                dict(reward=torch.ones(8, 2)[:, :1])):
        arguments = {**dict(reward=reward, returns=G, terminated=flags, truncated=flags, stats=stats, gamma=GAMMA, epsilon=EPSILON), **bad}
        with pytest.raises(ValueError, match="reward_normalize_"):
            ops.reward_normalize_cpu_(**arguments)
    with pytest.raises(ValueError, match="must be a CPU tensor"):
        ops.reward_normalize_cpu_(None, G, flags, flags, stats, GAMMA, EPSILON)


# ------------------------------------------------------------------------------------------------ the hook
def _transition(reward, terminated, truncated, t):
    return {"reward": torch.from_numpy(reward[t].copy()), "terminated": torch.from_numpy(terminated[t]).unsqueeze(-1),
            "truncated": torch.from_numpy(truncated[t]).unsqueeze(-1)}


def test_hook_host_form_is_the_op_and_its_state_loads_in_place(references):
    (reward, terminated, truncated), _ = references[(257, 2)]
    direct = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated, gamma=0.9, clip=2.0)
    hook = make_hook(cusrl, 257, 2, gamma=0.9, clip=2.0)
    assert type(hook).pre_act is cusrl.Hook.pre_act and type(hook).export_stages is cusrl.Hook.export_stages
    assert hook.rollout_capture_safe and not hook.step_draws_random and not hook.post_step_device_free
    assert hook.collective_phases() == () and hook.eager_phases() == ()
    statistics = hook.statistics
    assert statistics.returns.dtype == torch.float32 and statistics.stats.dtype == torch.float64
    assert statistics.stats.tolist() == [[0.0, 0.0], [1.0, 1.0], [1e-4, 1e-4]]
    addresses = statistics.returns.data_ptr(), statistics.stats.data_ptr()
    before = dict(_native.launch_counts)
    for t in range(3):
        transition = _transition(reward, terminated, truncated, t)
        hook.post_step(transition)
        assert torch.equal(transition["reward"], direct[t]["reward"])
        assert torch.equal(statistics.returns, direct[t]["returns"]) and torch.equal(statistics.stats, direct[t]["stats"])
    moved = {key: value - before.get(key, 0) for key, value in _native.launch_counts.items() if value != before.get(key, 0)}
    assert moved == {"cusrl_reward_normalize_cpu": 3}, moved
    saved = {key: (value.clone() if isinstance(value, torch.Tensor) else value) for key, value in _flat(hook.state_dict()).items()}
    assert set(saved) == {"statistics.returns", "statistics.stats", "hyper_parameters.gamma", "hyper_parameters.epsilon",
                          "hyper_parameters.clip", "hyper_parameters.update"}
    state = hook.state_dict()
    state = {"statistics": {key: value.clone() for key, value in state["statistics"].items()}, "hyper_parameters": state["hyper_parameters"]}
    other = make_hook(cusrl, 257, 2)  # other hyper-parameters, fresh statistics
    other_addresses = other.statistics.returns.data_ptr(), other.statistics.stats.data_ptr()
    other.load_state_dict(state)
    assert (other.gamma, other.epsilon, other.clip, other.update) == (0.9, 1e-8, 2.0, True)
    assert (other.statistics.returns.data_ptr(), other.statistics.stats.data_ptr()) == other_addresses
    for t in range(3, STEPS):  # both go on identically, and as the uninterrupted run
        a, b = _transition(reward, terminated, truncated, t), _transition(reward, terminated, truncated, t)
        hook.post_step(a)
        other.post_step(b)
        assert torch.equal(a["reward"], b["reward"]) and torch.equal(a["reward"], direct[t]["reward"])
        assert torch.equal(other.statistics.stats, direct[t]["stats"]) and torch.equal(other.statistics.returns, direct[t]["returns"])
    assert (statistics.returns.data_ptr(), statistics.stats.data_ptr()) == addresses


def _flat(state, lead=""):
    out = {}
    for key, value in state.items():
        out.update(_flat(value, f"{lead}{key}.") if isinstance(value, dict) else {f"{lead}{key}": value})
    return out


def test_hook_freezes_in_inference_mode_and_with_update_false(references):
    (reward, terminated, truncated), _ = references[(3, 1)]
    for freeze in ("update", "inference"):
        hook = make_hook(cusrl, 3, 1, update=freeze != "update")
        hook.agent.inference_mode = freeze == "inference"
        for t in range(2):
            hook.post_step(_transition(reward, terminated, truncated, t))
        assert hook.statistics.stats.tolist() == [[0.0], [1.0], [1e-4]] and hook._is_synchronized
        assert hook.statistics.returns.any()
    hook.update_attribute("update", True)
    hook.agent.inference_mode = False
    hook.post_step(_transition(reward, terminated, truncated, 2))
    assert hook.statistics.count.item() == 3.0001 and not hook._is_synchronized
    hook.pre_update(None)  # one rank: nothing to merge, nothing changes
    assert hook.statistics.count.item() == 3.0001


def test_hook_stages_a_reward_the_launch_does_not_take_and_checks_its_arguments(references):
    (reward, terminated, truncated), _ = references[(3, 1)]
    direct = run(ops.reward_normalize_cpu_, "cpu", reward, terminated, truncated)
    hook = make_hook(cusrl, 3, 1)
    transition = _transition(reward, terminated, truncated, 0)
    wide = torch.zeros(3, 2, dtype=torch.float64)
    wide[:, :1] = transition["reward"]
    transition["reward"] = wide[:, :1]  # float64 and strided
    hook.post_step(transition)
    assert torch.equal(wide[:, :1].float(), direct[0]["reward"]) and not wide[:, 1].any()
    for bad in (dict(gamma=1.5), dict(gamma=-0.1), dict(epsilon=-1.0), dict(clip=-1.0)):
        with pytest.raises(ValueError):
            cusrl.hook.RewardNormalization(**bad)
