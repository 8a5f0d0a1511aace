"""``cusrl_mlp2_forward`` (csrc/mlp_forward.hip) at all 16 instantiations ``<T1, T2, KB>``, every head width and every row edge,
and the one-output row dot ``cusrl_narrow_linear_fwd`` (csrc/narrow_linear.hip), on an MI355X.

An MFMA kernel cannot be restated bit for bit — the order of the sums inside the instruction is not ours to mirror — but it
can be pinned exactly on inputs for which every order gives the same fp32 result: the integer stacks of tests/_mlp_forward.py
(tests/test_mlp_forward_exact.py shows on the CPU that they are such inputs).  On them the assertion is ``torch.equal`` with
float64.  On random normals the kernel is held to four times the error the library's own fp32 chain makes on the same data,
both measured against float64 in the same test.  Rows must not depend on each other or on where they land in the grid (a
permutation of the rows permutes the output, bit for bit), the sampling epilogue must be ``cusrl_normal_sample_logp`` given
the same mean, and the raw entry point must write nothing outside its outputs."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _mlp_forward as M
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                  # floats on either side of an output (256 bytes: the output keeps its 16-byte alignment)
SENTINEL = 0x7FA5A5A5       # the bit pattern the guarded buffers are filled with (compared as int32)
HEADS = tuple(range(1, M.MAX_OUT + 1))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from cusrl_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def cus(ops) -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _launches() -> int:
    from cusrl_amd import _native

    return _native.launch_counts.get("cusrl_mlp2_forward", 0)


def _to_device(layers):
    return tuple(None if t is None else t.to(DEV) for t in layers)


def _integer_case(K, H1, H2, A, rows, seed, bias3=True):
    """The integer stack on the device and the float64 result every correct fp32 evaluation of it equals."""
    x, layers = M.integer_stack(K, H1, H2, A, rows, seed, bias3)
    return x.to(DEV), _to_device(layers), M.integer_expected(K, H1, H2, A, rows, seed, bias3)


def _normal(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _exact(ops, x, layers, want, label):
    assert ops.mlp2_forward_supported(x, layers), label
    before = _launches()
    out = ops.mlp2_forward(x, layers)
    assert _launches() == before + 1, f"{label}: one launch per call"
    assert out.shape == want.shape and out.dtype == torch.float32, label
    got = out.double().cpu()
    assert torch.equal(got, want), f"{label}: {int((got != want).sum())} of {want.numel()} elements differ, first at " \
                                   f"{(got != want).nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ 16 instantiations x 16 heads
@pytest.mark.parametrize("H1,H2,K", [(H1, H2, K) for H1, H2 in M.HIDDEN for K in M.K_EDGES],
                         ids=lambda v: str(v))
def test_integer_stack_is_exact_at_every_instantiation_and_head_width(ops, H1, H2, K):
    for bias3, heads in ((True, HEADS), (False, (1, 12, 16))):
        for A in heads:
            x, layers, want = _integer_case(K, H1, H2, A, M.ROWS_SMALL, 1, bias3)
            _exact(ops, x, layers, want, f"{M.instantiation(K, H1, H2)} {K}->{H1}->{H2}->{A}{'' if bias3 else ' without b3'}")


@pytest.mark.parametrize("K,H1,H2,A", [stack + (A,) for stack, A in zip(M.ROW_EDGE_STACKS, (12, 5))], ids=lambda v: str(v))
def test_integer_stack_is_exact_at_every_row_residue_and_grid_edge(ops, cus, K, H1, H2, A):
    """1..33 rows: a ragged single tile, exactly one and two tiles, one row into the next; 16 cus: the grid exactly full;
    16 cus + 1: workgroup 0 walks two tiles and its look-ahead load is clamped to the last one; 32 cus + 5: every workgroup
    walks more than one tile with the weights in place."""
    for rows in M.ROW_EDGES + M.grid_rows(cus):
        x, layers, want = _integer_case(K, H1, H2, A, rows, 2)
        _exact(ops, x, layers, want, f"{M.instantiation(K, H1, H2)} {K}->{H1}->{H2}->{A} at {rows} rows")


# ------------------------------------------------------------------------------------------------ rows are independent
@pytest.mark.parametrize("K,H1,H2,A", M.INDEPENDENCE_STACKS, ids=lambda v: str(v))
def test_rows_do_not_depend_on_their_place_in_the_grid(ops, cus, K, H1, H2, A):
    """A row is one column of the MFMA's N dimension: the order of its sums does not depend on the tile, lane or workgroup it
    lands in.  A permutation of the rows therefore permutes the output bit for bit; any difference is state leaking between
    rows or tiles (the LDS buffers re-used across the persistent loop, the one-tile-ahead input load, the epilogue's noise)."""
    rows = 32 * cus + 5
    layers = M.stack(K, H1, H2, A, seed=21, device=DEV)
    x, eps = _normal((rows, K), 22), _normal((rows, A), 23)
    std = (torch.rand(A, generator=torch.Generator().manual_seed(24)) * 0.9 + 0.1).to(DEV)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(25)).to(DEV)
    out = ops.mlp2_forward(x, layers)
    assert torch.equal(ops.mlp2_forward(x[perm].contiguous(), layers), out[perm])
    assert torch.equal(ops.mlp2_forward(x[:16].contiguous(), layers), out[:16]), "the first tile alone"
    action, logp, mean, _ = ops.mlp2_forward(x, layers, std=std, eps=eps)
    action_p, logp_p, mean_p, _ = ops.mlp2_forward(x[perm].contiguous(), layers, std=std, eps=eps[perm].contiguous())
    assert torch.equal(mean, out) and torch.equal(mean_p, out[perm])
    assert torch.equal(action_p, action[perm]) and torch.equal(logp_p, logp[perm])


# ------------------------------------------------------------------------------------------------ sampling epilogue
@pytest.mark.parametrize("which", range(3), ids=("1row", "17rows", "16cus+1rows"))
@pytest.mark.parametrize("K,H1,H2", M.SAMPLING_STACKS, ids=lambda v: str(v))
def test_sampling_epilogue_at_every_head_width(ops, cus, K, H1, H2, which):
    rows = M.sampling_rows(cus)[which]
    host = lambda t: t.cpu().numpy()  # noqa: E731
    for A in HEADS:
        label = f"{M.instantiation(K, H1, H2)} {K}->{H1}->{H2}->{A} at {rows} rows"
        # random normals: the epilogue is cusrl_normal_sample_logp given the same mean, and does not change the pass
        layers = M.stack(K, H1, H2, A, seed=30 + A, device=DEV)
        x, eps = _normal((rows, K), 31), _normal((rows, A), 32)
        std = (torch.rand(A, generator=torch.Generator().manual_seed(33)) * 0.9 + 0.1).to(DEV)
        action, logp, mean, repeated = ops.mlp2_forward(x, layers, std=std, eps=eps)
        assert torch.equal(mean, ops.mlp2_forward(x, layers)), label
        want_action, want_logp, want_repeated = ops.normal_sample_logp(mean, std, eps, repeat_std=True)
        assert torch.equal(action, want_action) and torch.equal(logp, want_logp) and torch.equal(repeated, want_repeated), label
        assert logp.shape == (rows, 1) and action.shape == repeated.shape == mean.shape == (rows, A), label
        assert np.array_equal(host(action), host(mean) + host(eps) * host(std)), label  # loc + eps * scale, separately rounded
        ref_logp, _ = oracle.normal_logp_entropy(host(action), host(mean), host(repeated))
        np.testing.assert_allclose(host(logp), ref_logp, rtol=1e-5, atol=1e-5, err_msg=label)
        # std_out = NULL: nothing else changes
        action_n, logp_n, mean_n, none = ops.mlp2_forward(x, layers, std=std, eps=eps, repeat_std=False)
        assert none is None and torch.equal(action_n, action) and torch.equal(logp_n, logp) and torch.equal(mean_n, mean), label
        # integers, integer noise and a power of two as std: mean + eps * std is exact, so the action is float64's
        x, layers, want_mean = _integer_case(K, H1, H2, A, rows, 3)
        rng = np.random.default_rng([rows, A])
        eps = torch.from_numpy(rng.integers(-2, 3, size=(rows, A)).astype(np.float32))
        std = torch.from_numpy(rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=A))
        want_action = want_mean + eps.double() * std.double()
        assert torch.equal(want_action.float().double(), want_action), "mean + eps * std is an fp32 value"
        action, logp, mean, repeated = ops.mlp2_forward(x, layers, std=std.to(DEV), eps=eps.to(DEV))
        assert torch.equal(mean.double().cpu(), want_mean) and torch.equal(action.double().cpu(), want_action), label
        assert torch.equal(repeated.cpu(), std.expand(rows, A)), label
        ref_logp, _ = oracle.normal_logp_entropy(host(action), host(mean), host(repeated))
        np.testing.assert_allclose(host(logp), ref_logp, rtol=1e-5, atol=1e-5, err_msg=label)


# ------------------------------------------------------------------------------------------------ nothing else is written
class _Guarded:
    """``numel`` floats between two guards of sentinel bits; ``offset`` floats shift the window off its 16-byte alignment."""

    def __init__(self, numel: int, offset: int = 0):
        self.first, self.numel = GUARD + offset, numel
        self.bits = torch.full((self.first + numel + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.ptr = self.bits.data_ptr() + 4 * self.first
        assert (self.ptr % 16 == 0) == (offset % 4 == 0)

    def check(self, want, label):
        bits = self.bits.cpu()
        assert bool((bits[:self.first] == SENTINEL).all()) and bool((bits[self.first + self.numel:] == SENTINEL).all()), \
            f"{label}: written outside the output"
        interior = bits[self.first:self.first + self.numel]
        if want is None:
            assert bool((interior == SENTINEL).all()), f"{label}: written although the call was refused"
        else:
            assert torch.equal(interior, want.contiguous().view(torch.int32).flatten().cpu()), f"{label}: the output itself"


@pytest.mark.parametrize("which", range(3), ids=("1row", "17rows", "16cus+1rows"))
def test_nothing_outside_the_outputs_is_written(ops, cus, which):
    from cusrl_amd import _native

    lib = _native.lib()
    rows = M.sampling_rows(cus)[which]
    K, H1, H2 = M.GUARD_STACK
    x = _normal((rows, K), 41)
    for A in M.GUARD_OUTS:
        layers = M.stack(K, H1, H2, A, seed=40 + A, device=DEV)
        eps = _normal((rows, A), 42)
        std = (torch.rand(A, generator=torch.Generator().manual_seed(43)) * 0.9 + 0.1).to(DEV)
        action, logp, mean, repeated = ops.mlp2_forward(x, layers, std=std, eps=eps)
        w1, b1, w2, b2, w3, b3 = (t.data_ptr() for t in layers)

        def call(out, sampled):
            bufs = [_Guarded(rows * A), _Guarded(rows), _Guarded(rows * A)] if sampled else [None, None, None]
            tail = [std.data_ptr(), eps.data_ptr()] + [b.ptr for b in bufs] if sampled else [None] * 5
            rc = lib.cusrl_mlp2_forward(x.data_ptr(), rows, K, w1, b1, H1, w2, b2, H2, w3, b3, A, out.ptr, *tail,
                                        torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return rc, bufs

        for offset in (0, 1):
            for sampled in (True, False):
                label = f"{K}->{H1}->{H2}->{A} at {rows} rows, out {4 * offset} bytes off, {'with' if sampled else 'without'} the epilogue"
                out = _Guarded(rows * A, offset)
                rc, bufs = call(out, sampled)
                accepted = offset == 0 or A % 4 != 0   # a misaligned out takes the scalar stores; the float4 form refuses it
                assert rc == (0 if accepted else M.UNSUPPORTED), label
                out.check(mean if accepted else None, label)
                if sampled:
                    for buf, want in zip(bufs, (action, logp, repeated)):
                        buf.check(want if accepted else None, label)


# ------------------------------------------------------------------------------------------------ random values
@pytest.mark.parametrize("H1,H2,K", [(H1, H2, K) for H1, H2 in M.HIDDEN for K in M.K_FLOAT], ids=lambda v: str(v))
def test_random_values_within_four_times_the_library_chains_own_error(ops, H1, H2, K):
    """The yardstick is the library's fp32 chain on the same data, not the kernel: a different but equally long fp32 summation
    order may be up to 4x as far from float64 (the allowance the reward-normalisation kernel has over its host form)."""
    rows, A = 1000, 12
    layers = M.stack(K, H1, H2, A, seed=50 + K, device=DEV)
    x = _normal((rows, K), 51)
    want, mag = M._reference(x, layers)
    e_lib = float(((M.library_chain(x, layers).double().cpu() - want).abs() / mag).max())
    e_kernel = float(((ops.mlp2_forward(x, layers).double().cpu() - want).abs() / mag).max())
    print(f"mlp2_forward {M.instantiation(K, H1, H2)} {K}->{H1}->{H2}->{A} x {rows}: kernel {e_kernel:.3e}, library chain {e_lib:.3e} "
          f"of the accumulated magnitude (ratio {e_kernel / e_lib:.2f})")
    assert e_lib > 0 and e_kernel <= 4 * e_lib, (e_kernel, e_lib)


# ------------------------------------------------------------------------------------------------ the one-output row dot
@pytest.mark.parametrize("K", M.ROW_DOT_KS)
def test_row_dot_forward_is_exact_on_integers_and_row_independent(ops, K):
    for rows in M.ROW_DOT_ROWS:
        for bias in (True, False):
            x, w, b = M.integer_row_dot(K, rows, 4, bias)
            want = M.row_dot_reference(x, w, b)
            x, w, b = x.to(DEV), w.to(DEV), None if b is None else b.to(DEV)
            assert ops.narrow_linear_forward_supported(x, w)
            out = ops.narrow_linear_forward(x, w, b)
            assert out.shape == (rows, 1) and torch.equal(out.double().cpu(), want), f"K={K}, {rows} rows, bias={bias}"
    rows = M.ROW_DOT_ROWS[-1]
    x, w, b = _normal((rows, K), 61), _normal((1, K), 62), _normal((1,), 63)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(64)).to(DEV)
    out = ops.narrow_linear_forward(x, w, b)
    assert torch.equal(ops.narrow_linear_forward(x[perm].contiguous(), w, b), out[perm])
    assert torch.equal(ops.narrow_linear_forward(x[:16].contiguous(), w, b), out[:16])
