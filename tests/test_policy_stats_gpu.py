"""``cusrl_policy_stats`` and ``cusrl_categorical_policy_stats`` (``csrc/policy_stats.hip``) and their shared finalize, held to
the float64 references of ``oracle``: every case of tests/_policy_stats.py through ``ops.policy_stats`` /
``ops.categorical_policy_stats`` and the shared assertions (tests/test_policy_stats.py runs the same cases through a float32
restatement and the same assertions without a GPU); then the C ABI called directly with guard elements behind every operand,
misaligned operands, the layouts ``OnPolicyStatistics`` supplies, determinism, argument errors and one check at hook level."""

import numpy as np
import pytest
import torch

import _policy_stats as P
import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 6  # elements behind every operand that no launch may touch (two rows of partials)
SENTINEL = -1234.5
INVALID = -1  # CUSRL_E_INVALID
ENTRY = {"gaussian": "cusrl_policy_stats", "categorical": "cusrl_categorical_policy_stats"}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from cusrl_amd import ops as _ops

    return _ops


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(ops, case, tensors):
    return (ops.categorical_policy_stats if case.family == "categorical" else ops.policy_stats)(*tensors)


@pytest.mark.parametrize("case", P.CASES, ids=lambda case: case.name)
def test_statistics_against_float64(ops, case):
    from cusrl_amd import _native

    before = _native.launch_counts.get(ENTRY[case.family], 0)
    got = host(launch(ops, case, [dev(x) for x in P.operands(case, P.inputs(case))]))
    assert _native.launch_counts.get(ENTRY[case.family], 0) == before + 1
    P.check(case, got)


# ------------------------------------------------------------------------------------------------ the C ABI, guarded
class Raw:
    """One direct call of the C entry point.  Every operand is a fresh device copy inside an allocation of its own with
    sentinel elements behind it (``offset``: the named float operands start one float into their allocation — not 16-byte
    aligned); ``partials`` (NaN before the launch) and ``out`` likewise.  After the launch the sentinels and every read-only
    operand must be bit-identical, and ``partials`` must hold exactly ``num_partials(B)`` written rows."""

    def __init__(self, offset=()):
        self.offset = set(offset)

    def place(self, name, array, count=None, dtype=torch.float32):
        count = array.size if array is not None else count
        lead = 1 if name in self.offset else 0
        buffer = torch.full((lead + count + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        view = buffer[lead:lead + count]
        view.copy_(torch.from_numpy(array.reshape(-1))) if array is not None else view.fill_(float("nan"))
        if dtype == torch.float32:
            assert view.data_ptr() % 16 == (4 if lead else 0)
        self.placed[name] = (buffer, view, lead, None if array is None else array.copy())
        return view

    def run(self, case, data):
        from cusrl_amd import _native

        lib = _native.lib()
        self.placed = {}
        B, A, D = case.B, case.A, case.D
        rows = int(lib.cusrl_policy_stats_num_partials(B))
        assert rows == P.num_partials(B)
        names = P.OPERANDS[case.family]
        pointers = [self.place(name, data[name]).data_ptr() for name in names]
        partials = self.place("partials", None, rows * 3, torch.float64)
        out = self.place("out", None, 3)
        status = getattr(lib, ENTRY[case.family])(*pointers, B, A, D, partials.data_ptr(), out.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert status == 0, status
        for name, (buffer, view, lead, original) in self.placed.items():
            whole = host(buffer)
            assert (whole[:lead] == SENTINEL).all() and (whole[whole.size - GUARD:] == SENTINEL).all(), f"{name}: wrote out of bounds"
            if original is not None:
                assert np.array_equal(bits(host(view)), bits(original.reshape(-1))), f"{name}: a read-only operand changed"
        written = host(partials).reshape(rows, 3)
        assert not np.isnan(written).any(), f"{case.name}: partial rows left unwritten: {np.nonzero(np.isnan(written).any(1))[0]}"
        return host(out), written


@pytest.mark.parametrize("family", ["categorical", "gaussian"])
@pytest.mark.parametrize("B", [1, 257, 65537])
def test_c_abi_stays_inside_its_operands(family, B):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    case = P.find(family, "far", B, {257: 18 if family == "categorical" else 12}.get(B))
    data = P.inputs(case)
    out, partials = Raw().run(case, data)
    P.check(case, out)
    # the finalize: out = sum of the partial rows over B, B * D, B * A
    sums = partials.sum(0)
    want = np.array([sums[0] / B, sums[1] / (B * case.D), sums[2] / (B * case.A)])
    np.testing.assert_allclose(out, want, rtol=2e-7, atol=0.0)
    if family == "categorical":
        assert not partials[:, 2].any()
    else:  # block ownership: partial row k holds the rows [256 k, 256 (k + 1))
        std = data["new_std"].astype(np.float64).sum(-1)
        blocks = np.add.reduceat(std, np.arange(0, B, P.BLOCK))
        np.testing.assert_allclose(partials[:, 2], blocks, rtol=1e-6)


@pytest.mark.parametrize("family", ["categorical", "gaussian"])
def test_misaligned_operands_give_the_same_bits(family):
    """B = 257 with, in turn, each float operand (and ``out``) — then all of them — starting one float into its allocation."""
    assert torch.cuda.is_available(), "these tests need an MI355X"
    case = P.find(family, "far", 257, 18 if family == "categorical" else 12)
    data = P.inputs(case)
    aligned, partials = Raw().run(case, data)
    P.check(case, aligned)
    names = P.OPERANDS[family] + ("out",)
    for offset in [(name,) for name in names] + [names]:
        got, got_partials = Raw(offset).run(case, data)
        assert np.array_equal(bits(got), bits(aligned)), (family, offset, got, aligned)
        assert np.array_equal(got_partials.view(np.uint64), partials.view(np.uint64)), (family, offset)


# ------------------------------------------------------------------------------------------------ layouts from the hook
@pytest.mark.parametrize("family", ["categorical", "gaussian"])
def test_layouts_of_the_hook_give_the_same_bits(ops, family):
    """Flat [B, A] operands; the same data as [T, N, A] with ``old_logp`` [T, N, 1] and ``advantage`` [T, N, D] (a temporal
    batch); and a transposed [N, T, A] tensor per operand (non-contiguous: the wrapper makes it contiguous)."""
    T, N = 8, 32
    case = P.find(family, "far", T * N)
    A, D = case.A, case.D
    flat = [dev(x) for x in P.operands(case, P.inputs(case))]
    want = host(launch(ops, case, flat))
    P.check(case, want)

    def temporal(t):
        return t.view(T, N, -1)

    def transposed(t):
        view = temporal(t).transpose(0, 1).contiguous().transpose(0, 1)  # [T, N, .] over [N, T, .] storage
        assert not view.is_contiguous() and torch.equal(view, temporal(t))
        return view

    for layout in (temporal, transposed):
        tensors = [layout(t) for t in flat]
        assert tensors[0].shape == (T, N, A) and tensors[-2].shape == (T, N, 1) and tensors[-1].shape == (T, N, D)
        got = host(launch(ops, case, tensors))
        assert np.array_equal(bits(got), bits(want)), (family, layout.__name__, got, want)
    mixed = [transposed(t) if i % 2 else t for i, t in enumerate(flat)]  # flat and non-contiguous operands in one call
    assert np.array_equal(bits(host(launch(ops, case, mixed))), bits(want))


def test_an_expanded_std_vector_gives_the_bits_of_the_matrix(ops):
    """``new_std`` as the actor's [A] vector expanded over the rows (stride 0), flat and in the temporal layout."""
    T, N = 8, 32
    case = P.find("gaussian", "far", T * N)
    data = P.inputs(case)
    vector = dev(data["new_std"][0])
    matrix = vector.expand(case.B, case.A)
    assert matrix.stride() == (0, 1)
    data["new_std"] = np.broadcast_to(data["new_std"][0], (case.B, case.A)).copy()
    data["old_logp"] = (P._normal_logp(data["action"], data["new_mean"], data["new_std"]) + 0.5).astype(np.float32)
    tensors = [dev(x) for x in P.operands(case, data)]
    want = host(ops.policy_stats(*tensors))
    reference, mass = oracle.policy_stats(*P.operands(case, data), return_mass=True)
    assert all(abs(float(want[k]) - reference[k]) <= P.RELATIVE * mass[k] for k in range(3)), (want, reference, mass)
    tensors[3] = matrix
    assert np.array_equal(bits(host(ops.policy_stats(*tensors))), bits(want))
    temporal = [t.view(T, N, -1) for t in tensors[:3]] + [vector.expand(T, N, case.A)] + [t.view(T, N, -1) for t in tensors[4:]]
    assert temporal[3].stride() == (0, 0, 1)
    assert np.array_equal(bits(host(ops.policy_stats(*temporal))), bits(want))


@pytest.mark.parametrize("family", ["categorical", "gaussian"])
def test_two_launches_give_identical_bits(ops, family):
    """Fixed summation order: B = 70001 (274 partial rows, a ragged last workgroup), twice on the same inputs."""
    case = P.find(family, "far", 70001)
    tensors = [dev(x) for x in P.operands(case, P.inputs(case))]
    first = launch(ops, case, tensors).clone()
    scratch = torch.full((1 << 20,), float("nan"), device=DEV)  # (recycle the allocator's blocks with other contents)
    del scratch
    second = launch(ops, case, tensors)
    assert np.array_equal(bits(host(first)), bits(host(second))), (host(first), host(second))
    P.check(case, host(first))


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("family", ["categorical", "gaussian"])
def test_wrapper_argument_errors(ops, family):
    case = P.find(family, "far", 63)
    good = [dev(x) for x in P.operands(case, P.inputs(case))]
    fn = ops.categorical_policy_stats if family == "categorical" else ops.policy_stats
    B, A, D = case.B, case.A, case.D

    def replaced(index, tensor):
        return [tensor if i == index else t for i, t in enumerate(good)]

    n = len(good)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*replaced(n - 2, torch.zeros(B + 1, device=DEV)))  # old_logp
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*replaced(n - 1, torch.zeros(B * D + 1, device=DEV)))  # advantage: no whole number of columns
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*replaced(0, torch.zeros(B, A + 1, device=DEV)))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*replaced(n - 3, torch.zeros(B - 1, A, device=DEV)))  # action
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*replaced(n - 1, torch.zeros(B, 0, device=DEV)))  # D = 0
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*(torch.zeros(0, A, device=DEV) for _ in range(n - 2)), torch.zeros(0, device=DEV), torch.zeros(0, D, device=DEV))  # B = 0
    with pytest.raises(ValueError, match="inconsistent shapes"):
        fn(*(torch.zeros(B, 0, device=DEV) for _ in range(n - 2)), torch.zeros(B, device=DEV), torch.zeros(B, D, device=DEV))  # A = 0
    for index in range(n):
        with pytest.raises(TypeError, match="must be float32"):
            fn(*replaced(index, good[index].double()))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*replaced(index, good[index].cpu()))
    P.check(case, host(fn(*good)))  # (and the operands are still good)


@pytest.mark.parametrize("family", ["categorical", "gaussian"])
def test_c_abi_refuses_empty_sizes_and_null_pointers_without_launching(family):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from cusrl_amd import _native

    lib = _native.lib()
    entry = getattr(lib, ENTRY[family])
    operands = len(P.OPERANDS[family])
    B, A, D = 5, 3, 2
    inputs = [torch.ones(B * A, device=DEV) for _ in range(operands)]
    partials = torch.full((8, 3), SENTINEL, dtype=torch.float64, device=DEV)
    out = torch.full((3,), SENTINEL, device=DEV)
    pointers = [t.data_ptr() for t in inputs] + [partials.data_ptr(), out.data_ptr()]
    stream = torch.cuda.current_stream().cuda_stream

    def call(pointers, B, A, D):
        return entry(*pointers[:operands], B, A, D, pointers[operands], pointers[operands + 1], stream)

    for sizes in ((0, A, D), (B, 0, D), (B, A, 0), (-1, A, D), (B, -1, D), (B, A, -1), (B, 2**31, D), (B, A, 2**31)):
        assert call(pointers, *sizes) == INVALID, sizes
    for index in range(len(pointers)):
        assert call([None if i == index else p for i, p in enumerate(pointers)], B, A, D) == INVALID, index
    assert lib.cusrl_policy_stats_num_partials(0) == 0 and lib.cusrl_policy_stats_num_partials(-3) == 0
    torch.cuda.synchronize()
    assert bool((partials == SENTINEL).all()) and bool((out == SENTINEL).all()), "a refused call wrote its outputs"
    assert call(pointers, B, A, D) == 0  # (and the same pointers are accepted with valid sizes)
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).all()) and bool((partials[1:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ at hook level
def test_the_hook_records_what_float64_torch_distributions_give(ops, monkeypatch):
    """A small categorical PPO agent (64 envs, 8 steps, observation 6, 5 actions, eager), one update: the batch the hook hands
    to ``ops.categorical_policy_stats``, recomputed with float64 torch.distributions on the host, is what ``last_info`` holds."""
    import cusrl_amd as cusrl
    from torch.distributions import OneHotCategorical, kl_divergence

    cusrl.config.set_device(DEV)
    cusrl.set_global_seed(11)
    seen = []
    original = ops.categorical_policy_stats

    def spy(*tensors):
        seen.append([t.detach().clone() for t in tensors])
        return original(*tensors)

    monkeypatch.setattr(cusrl.ops, "categorical_policy_stats", spy)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=64, observation_dim=6, action_dim=5, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, actor_hidden_dims=(32, 32), critic_hidden_dims=(32, 32),
                                           action_space_type="discrete", sampler_epochs=2, sampler_mini_batches=2)
    trainer = cusrl.Trainer(env, factory, num_iterations=1, verbose=False)
    trainer.run_training_loop()
    info = trainer.last_info
    assert len(seen) == 1, "one update, one batch of the whole buffer"
    batch = seen[0]
    old_logits, new_logits, action, old_logp, advantage = (host(t).astype(np.float64) for t in batch)
    rows = 64 * 8
    assert old_logits.size == rows * 5 and old_logp.size == rows and advantage.size == rows
    assert not np.array_equal(old_logits, new_logits), "the update left the actor where it was"
    t = lambda a, width: torch.from_numpy(a.reshape(rows, width))  # noqa: E731
    p, q = OneHotCategorical(logits=t(old_logits, 5)), OneHotCategorical(logits=t(new_logits, 5))
    kl = kl_divergence(p, q).unsqueeze(-1).mean().item()
    weighted = (t(advantage, 1) * (q.log_prob(t(action, 5)).unsqueeze(-1) - t(old_logp, 1)).exp()).mean().item()
    restated, mass = oracle.categorical_policy_stats(old_logits, new_logits, action, old_logp, advantage, return_mass=True)
    assert abs(restated[0] - kl) <= 1e-12 * mass[0] and abs(restated[1] - weighted) <= 1e-12 * mass[1]
    direct = host(original(*batch))
    assert direct[2] == 0.0
    for label, got in (("ops", direct[:2]), ("last_info", (info["Agent/kl_divergence"], info["Agent/importance_weighted_advantage"]))):
        for k, want in enumerate((kl, weighted)):
            error, bound = abs(float(got[k]) - want), P.RELATIVE * mass[k]
            print(f"hook/{label}:{P.STATISTICS[k]}: |got - float64| = {error:.3e}, bound {bound:.3e}")
            assert error <= bound, f"{label}:{P.STATISTICS[k]}: {float(got[k])!r} vs {want!r}: off by {error:.3e} > {bound:.3e}"
    assert "Agent/action_std" not in info
