"""``cusrl_nan_to_num2`` and ``ObservationNanToNum`` on the GPU.  Every comparison is bit-exact on integer views: the operation
only selects values.  Kernel level: against ``torch.nan_to_num`` of the same data on the CPU, with guard elements around every
view (the launch takes offset views: 4-byte alignment only).  In the loop: an env that writes NaN / +Inf / -Inf into fixed
``(step, env, column)`` positions of the observation it returns, host-driven against captured."""

import numpy as np
import pytest
import torch

from test_nan_to_num import PARAMETER_SETS, SPECIALS, replay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = "cusrl_nan_to_num2"
SPAN = 256 * 2 * 4        # elements of one array one block covers per pass (kSanitizeSpan)
CAP = 2048                # blocks (kSanitizeMaxBlocks)
GUARD = 0x7FC0BEEF        # a NaN pattern no parameter set produces: a guard element that was written is no longer this
# 1..1027: scalar-only arrays, one body vector with / without head and tail, the block size and around it; SPAN - 6 .. : the
# last length of one block, the first of two; CAP * SPAN + ...: the first length at which a thread makes a second pass
LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1027, SPAN - 6, SPAN - 5, SPAN + 9, CAP * SPAN + SPAN + 5)


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name=KERNEL):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def bits_of(n, seed, specials=True):
    """``n`` ordinary N(0, 3) values as int32 bits; with ``specials`` about one element in seven is one of the ten."""
    generator = torch.Generator().manual_seed(seed)
    bits = (3.0 * torch.randn(n, generator=generator)).view(torch.int32)
    if specials and n:
        where = torch.rand(n, generator=generator) < 0.15
        pick = torch.randint(0, len(SPECIALS), (n,), generator=generator)
        table = torch.tensor(SPECIALS, dtype=torch.int64).to(torch.int32)  # (wraps the patterns with the sign bit set)
        bits = torch.where(where, table[pick], bits)
    return bits


def reference(bits, params):
    nan, posinf, neginf = params
    return torch.nan_to_num(bits.view(torch.float32), nan=nan, posinf=posinf, neginf=neginf).view(torch.int32)


def guarded(bits, offset):
    """A device view ``base[offset : offset + n]`` of the data with ``offset`` guard elements in front and 4 behind."""
    base = torch.full((offset + bits.numel() + 4,), GUARD, dtype=torch.int64).to(torch.int32)
    base[offset:offset + bits.numel()] = bits
    base = base.to(DEV)
    return base, base[offset:offset + bits.numel()].view(torch.float32)


def check(ops, a_bits, b_bits, params, ka=0, kb=0):
    nan, posinf, neginf = params
    base_a, a = guarded(a_bits, ka)
    base_b, b = (None, None) if b_bits is None else guarded(b_bits, kb)
    assert a.data_ptr() % 16 == (4 * ka) % 16
    before = _count()
    out = ops.nan_to_num_(a, b, nan=nan, posinf=posinf, neginf=neginf)
    assert out is a and _count() == before + 1
    for base, bits, k in ((base_a, a_bits, ka), (base_b, b_bits, kb)):
        if base is None:
            continue
        got = base.cpu()
        assert torch.equal(got[k:k + bits.numel()], reference(bits, params)), (bits.numel(), k, params)
        guards = torch.cat([got[:k], got[k + bits.numel():]]).to(torch.int64) & 0xFFFFFFFF
        assert bool((guards == GUARD).all()), (bits.numel(), k)  # nothing outside the view was written


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_alignments_match_torch(cusrl, n):
    from cusrl_amd import ops

    a_bits = bits_of(n, seed=n)
    check(ops, a_bits, None, PARAMETER_SETS["finite"])
    if n >= 5:  # 4-byte but not 16-byte aligned views, another offset for b than for a
        b_bits = bits_of(min(n, 1027) + 2, seed=n + 1)
        for ka, kb in ((1, 3), (2, 1), (3, 2)):
            check(ops, a_bits, b_bits, PARAMETER_SETS["finite"], ka, kb)


def test_second_array_absent_empty_shorter_longer(cusrl):
    from cusrl_amd import ops

    a_bits = bits_of(300, seed=5)
    for params in PARAMETER_SETS.values():
        check(ops, a_bits, None, params)
        check(ops, a_bits, bits_of(0, seed=6), params)           # empty
        check(ops, a_bits, bits_of(41, seed=7), params, 0, 1)    # shorter
        check(ops, a_bits, bits_of(2600, seed=8), params, 2, 0)  # longer: b alone decides the grid (two blocks)
    empty = torch.empty(0, device=DEV)
    before = _count()
    assert ops.nan_to_num_(empty, None) is empty and ops.nan_to_num_(empty, torch.empty(0, device=DEV)) is empty
    assert _count() == before + 2  # (the entry point was asked; with nothing to do it returns before any launch)


@pytest.mark.parametrize("set_name", list(PARAMETER_SETS))
def test_every_special_at_every_boundary(cusrl, set_name):
    """Each of the ten specials at element 0, at the last element, in each of the four lanes of a body vector and on both sides
    of the head / body and body / tail boundaries — for a view 1, 2 and 3 elements past a 16-byte boundary (heads of 3, 2, 1)
    and an aligned one (no head)."""
    from cusrl_amd import ops

    for k in (0, 1, 2, 3):
        head = (4 - k) % 4
        n = head + 10 * 4 + 2  # ten body vectors and a tail of two behind the head
        tail = n - 2
        places = sorted({0, n - 1, max(head - 1, 0), head, head + 4, head + 5, head + 6, head + 7, tail - 1, tail})
        for rotation in range(len(SPECIALS)):
            a_bits, b_bits = bits_of(n, seed=rotation, specials=False), bits_of(n, seed=100 + rotation, specials=False)
            table = torch.tensor(np.roll(SPECIALS, rotation), dtype=torch.int64).to(torch.int32)
            a_bits[places] = table[: len(places)]
            b_bits[places] = table[: len(places)].flip(0)
            check(ops, a_bits, b_bits, PARAMETER_SETS[set_name], k, (k + 1) % 4)


def test_clean_input_is_untouched_and_all_nan_input_is_replaced_everywhere(cusrl):
    from cusrl_amd import ops

    for n, k in ((1027, 0), (1027, 3), (2 * SPAN + 3, 1)):
        clean = bits_of(n, seed=n, specials=False)
        finite_specials = torch.tensor([s for s in SPECIALS if (s & 0x7F800000) != 0x7F800000], dtype=torch.int64).to(torch.int32)
        clean[:: 7] = finite_specials[torch.arange(clean[:: 7].numel()) % finite_specials.numel()]  # -0.0, denormals, +-FLT_MAX
        base, view = guarded(clean, k)
        ops.nan_to_num_(view, nan=1.5, posinf=2.0, neginf=3.0)
        assert torch.equal(base.cpu()[k:k + n], clean)  # output bits = input bits
        nans = torch.tensor([0x7FC00000, 0x7FA00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=torch.int64).to(torch.int32)
        dirty = nans[torch.arange(n) % nans.numel()]
        base, view = guarded(dirty, k)
        ops.nan_to_num_(view, nan=1.5, posinf=2.0, neginf=3.0)
        assert bool((base.cpu()[k:k + n].view(torch.float32) == 1.5).all())
        check(ops, dirty, dirty.clone(), PARAMETER_SETS["defaults"], k, (k + 2) % 4)


def test_error_returns_and_contract_checks(cusrl):
    from cusrl_amd import _native, ops

    lib = _native.lib()
    x = torch.zeros(16, device=DEV)
    assert lib.cusrl_nan_to_num2(x.data_ptr(), -1, None, 0, 0.0, 0.0, 0.0, None) == -1   # negative count
    assert lib.cusrl_nan_to_num2(x.data_ptr(), 16, x.data_ptr(), -4, 0.0, 0.0, 0.0, None) == -1
    assert lib.cusrl_nan_to_num2(None, 16, None, 0, 0.0, 0.0, 0.0, None) == -1           # null a with na > 0
    assert lib.cusrl_nan_to_num2(x.data_ptr(), 16, None, 3, 0.0, 0.0, 0.0, None) == -1   # null b with nb > 0
    with pytest.raises(TypeError):
        ops.nan_to_num_(torch.zeros(4, 4, device=DEV).t())
    with pytest.raises(TypeError):
        ops.nan_to_num_(x, torch.zeros(4, device=DEV, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.nan_to_num_(torch.zeros(4, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nan_to_num_(torch.zeros(4))


def test_hook_fallbacks_equal_torch(cusrl):
    hook = cusrl.hook.ObservationNanToNum(1.5, 1e6, -1e6)
    specials = torch.tensor(SPECIALS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    values = torch.cat([specials, torch.randn(30, generator=torch.Generator().manual_seed(2))]).reshape(8, 5)
    cases = {
        "transposed": (values.clone(), lambda t: t.t(), torch.int32, 1),
        "bf16": (values.to(torch.bfloat16), lambda t: t, torch.int16, 1),
        "fp16": (values.to(torch.float16), lambda t: t, torch.int16, 1),
        # float64 stays on torch: an fp32 copy would round it (1e300 would even become an infinity)
        "float64": (torch.cat([values.double().reshape(-1), torch.tensor([1e300, -1e-310, 1.0 + 2.0 ** -40])]), lambda t: t, torch.int64, 0),
        "int32": (torch.arange(-5, 5, dtype=torch.int32), lambda t: t, torch.int32, 0),
    }
    for name, (cpu, view, as_int, launches) in cases.items():
        device_base = cpu.clone().to(DEV)
        expected = view(cpu.clone()).nan_to_num_(nan=1.5, posinf=1e6, neginf=-1e6)
        before = _count()
        hook.post_step({"next_observation": view(device_base)})
        assert _count() - before == launches, name
        got = view(device_base).cpu()
        assert torch.equal(got.contiguous().view(as_int), expected.contiguous().view(as_int)), name
    # both fields of one call share ONE launch, whichever of them had to be staged
    transition = {"observation": values.clone().to(DEV), "state": values.to(torch.bfloat16).to(DEV)}
    before = _count()
    hook.pre_act(transition)
    assert _count() - before == 1
    assert torch.isfinite(transition["observation"]).all() and torch.isfinite(transition["state"].float()).all()
    with pytest.raises(RuntimeError, match="CPU tensors"):  # the gate of the host form is shut in a GPU test
        hook.pre_act({"observation": values.clone()})


def test_hook_on_the_gpu_reproduces_every_recorded_case(cusrl, golden):
    g = golden("nan_to_num")
    for case in map(str, g["cases"]):
        before = _count()
        got, want = replay(g, case, device=DEV)
        assert _count() - before == 2, case  # pre_act and post_step: one launch each, with or without a state
        for field in want:
            assert np.array_equal(got[field], want[field]), (case, field)


# ------------------------------------------------------------------------------------------------ in the loop
N, OBS, ACT, T = 64, 16, 8, 8
PARAMS = (1.5, 1e6, -1e6)
# (step, env, column) -> what the env writes there
INJECTED = {(0, 0, 0): float("nan"), (0, N - 1, OBS - 1): float("inf"), (2, 5, 3): float("-inf"), (3, 17, 7): float("nan"),
            (5, 40, 0): float("inf"), (T - 1, 63, 9): float("-inf"), (T - 1, 0, 15): float("nan")}
REPLACED = {float("inf"): PARAMS[1], float("-inf"): PARAMS[2]}


def poisoned_environment(cusrl, state_dim=None):
    """The dummy env whose returned observation carries the INJECTED values at step ``t mod T`` (a device-side counter: the
    same launches whether the step runs eagerly or is replayed from a graph; nothing drawn from a generator), which logs the
    observation it had before, and whose first reset row carries a NaN (what ``pre_act`` meets at the next act step)."""

    class Poisoned(cusrl.testing.DummyTorchEnvironment):
        def __init__(self):
            super().__init__(num_instances=N, observation_dim=OBS, action_dim=ACT, state_dim=state_dim, device=DEV)
            where, value = torch.zeros(T, N, OBS, dtype=torch.bool), torch.zeros(T, N, OBS)
            for (t, n, c), v in INJECTED.items():
                where[t, n, c], value[t, n, c] = True, v
            self.where, self.value = where.to(DEV), value.to(DEV)
            self.t = torch.zeros(1, dtype=torch.int64, device=DEV)
            self.clean = torch.zeros(T, N, OBS, device=DEV)
            self.reset_where = torch.zeros(N, OBS, dtype=torch.bool, device=DEV)
            self.reset_where[0, 3] = True
            self.nan = torch.full((), float("nan"), device=DEV)

        def step(self, action):
            observation, *rest = super().step(action)
            self.clean.index_copy_(0, self.t, observation.unsqueeze(0))
            poisoned = torch.where(self.where.index_select(0, self.t)[0], self.value.index_select(0, self.t)[0], observation)
            self.t.add_(1).remainder_(T)
            return (poisoned, *rest)

        def reset_static(self, indices, count):
            observation, state, info = super().reset_static(indices, count)
            return torch.where(self.reset_where, self.nan, observation), state, info

    return Poisoned()


def rollouts(cusrl, compile_, iterations, *, hook=True, state_dim=None, snapshots=(), capture=True):
    """``iterations`` rollouts + updates of the smallest preset agent on the poisoned env from one seed; the same (fused,
    capturable) Adam whether ``compile_`` or not; ``capture=False`` keeps a compile=True trainer's rollout host-driven."""
    cusrl.set_global_seed(13)
    env = poisoned_environment(cusrl, state_dim)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=T, sampler_epochs=2, sampler_mini_batches=2, compile=compile_,
                                           optimizer_kwargs={"capturable": True, "fused": True}).to_underlying()
    if hook:
        factory.register_hook(cusrl.hook.ObservationNanToNum(*PARAMS), index=0)  # first in the list
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    trainer.capture_rollout = capture
    observation, state, _ = env.reset(randomize_episode_progress=True)
    taken = {}
    for iteration in range(1, iterations + 1):
        observation, state = trainer._rollout_and_update(observation, state)
        trainer.iteration += 1
        if iteration in snapshots:
            torch.cuda.synchronize()
            taken[iteration] = ({key: leaf.clone() for key, leaf in trainer.agent.buffer.storage.items()},
                                {name: p.detach().clone() for name, p in trainer.agent.named_parameters()})
    trainer.flush()
    return trainer, env, taken


def differences(one, other):
    """``{name: largest absolute difference}`` over the entries of two snapshots that are not bit-identical."""
    found = {}
    for group_a, group_b in zip(one, other):
        assert set(group_a) == set(group_b)
        for name, a in group_a.items():
            if not int_equal(a, group_b[name]):
                found[name] = float((a.double() - group_b[name].double()).abs().max())
    return found


def int_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def test_rollout_buffer_is_sanitised_and_everything_else_is_the_envs_value(cusrl):
    from cusrl_amd import _native

    before = dict(_native.launch_counts)
    trainer, env, _ = rollouts(cusrl, False, 1)
    # host-driven: 2 T calls of the entry point over a rollout of T steps — pre_act and post_step, one launch each
    assert _native.launch_counts[KERNEL] - before.get(KERNEL, 0) == 2 * T
    buffer = trainer.agent.buffer
    observation, next_observation = buffer["observation"], buffer["next_observation"]
    assert torch.isfinite(observation).all() and torch.isfinite(next_observation).all()
    expected = env.clean.clone()
    for (t, n, c), value in INJECTED.items():
        expected[t, n, c] = PARAMS[0] if value != value else REPLACED[value]
    assert int_equal(next_observation, expected)  # the injected positions replaced, every other entry the env's bits
    # the next act input: the sanitised next observation, reset rows spliced in for the finished envs (their NaN met pre_act)
    done = (buffer["terminated"] | buffer["truncated"]).squeeze(-1)
    assert done[:-1].any()
    kept = ~done[:-1]
    assert int_equal(observation[1:][kept], next_observation[:-1][kept])
    # Without the hook one non-finite observation reaches every parameter through the next update; with it they stay finite
    assert all(torch.isfinite(p).all() for p in trainer.agent.parameters())
    unprotected, _, _ = rollouts(cusrl, False, 1, hook=False)
    assert not all(torch.isfinite(p).all() for p in unprotected.agent.parameters())


def test_state_shares_the_observations_launch(cusrl):
    from cusrl_amd import _native

    before = dict(_native.launch_counts)
    trainer, env, _ = rollouts(cusrl, False, 1, state_dim=5)
    assert trainer.agent.has_state and "state" in trainer.agent.buffer.storage
    assert _native.launch_counts[KERNEL] - before.get(KERNEL, 0) == 2 * T  # still one launch per hook call
    assert torch.isfinite(trainer.agent.buffer["next_observation"]).all()


def test_captured_rollout_with_the_hook_replays_and_is_bit_identical_to_the_host_driven_loop(cusrl):
    """compile=True both times.  Iteration 0 is host-driven, 1 runs the step bodies eagerly, 2 captures every step and replays
    it, 3 captures the whole rollout as one graph and replays that; the other trainer keeps the host-driven loop throughout."""
    host, _, host_taken = rollouts(cusrl, True, 4, snapshots=(2, 4), capture=False)
    captured, env, captured_taken = rollouts(cusrl, True, 4, snapshots=(2, 4))
    assert host._graphed_rollout is None
    graphed = captured._graphed_rollout
    # the hook does not keep the agent off the captured rollout: every step has its graph, the whole rollout one on top
    assert graphed is not None and graphed.captured == T and len(graphed.rollouts) == 1, (graphed and graphed.captured)
    assert captured.environment.generator_free
    for iteration in (2, 4):
        found = differences(host_taken[iteration], captured_taken[iteration])
        print(f"captured vs host-driven after {iteration} iterations: {found or 'bit-identical'}")
        assert not found, (iteration, found)
        leaves, parameters = captured_taken[iteration]
        assert all(torch.isfinite(p).all() for p in parameters.values())
        assert torch.isfinite(leaves["observation"]).all() and torch.isfinite(leaves["next_observation"]).all()
    last = captured_taken[4][0]["next_observation"]  # the replayed whole-rollout graph sanitised what the env wrote
    for (t, n, c), value in INJECTED.items():
        assert float(last[t, n, c]) == (PARAMS[0] if value != value else REPLACED[value])


def test_two_iterations_under_compile_and_eager_are_bit_identical(cusrl):
    """Two iterations with compile=True and two with compile=False from the same seed: buffer contents and parameters."""
    _, _, eager = rollouts(cusrl, False, 2, snapshots=(2,))
    _, _, compiled = rollouts(cusrl, True, 2, snapshots=(2,))
    found = differences(eager[2], compiled[2])
    print(f"compile=True vs compile=False after 2 iterations: {found or 'bit-identical'}")
    assert all(torch.isfinite(p).all() for p in compiled[2][1].values())
    assert not found, found
