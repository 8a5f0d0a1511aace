"""``cusrl_mlp2_wave_forward`` (csrc/mlp2_wave_forward.hip) on an MI355X: exact on integer stacks, within four times the library
chain's own error on random values, row-independent, the same bits from both read paths, ``cusrl_normal_sample_logp`` behind the
same mean, and guarded — through ``ops.mlp2_wave_forward``, the interface the pass is reached from."""

from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from cusrl_amd import _native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = ((64, 64), (32, 64), (64, 32), (32, 32))
ACT = {"ReLU": torch.relu, "ELU": F.elu, "Tanh": torch.tanh}
UNSUPPORTED = -3                   # CUSRL_E_UNSUPPORTED
GUARD, SENTINEL = 64, 0x7FA5A5A5   # floats on either side of a guarded output, and the bits they hold


def _launches() -> int:
    return _native.launch_counts.get("cusrl_mlp2_wave_forward", 0)


def _reference(x, layers, activation):
    """float64 ``(out, mag)``: the stack and the magnitude its fp32 sums accumulate."""
    h, mag = x.double().cpu(), x.double().cpu().abs()
    for n, (weight, bias) in enumerate(zip(layers[0::2], layers[1::2])):
        weight = weight.double().cpu()
        h, mag = h @ weight.T, mag @ weight.abs().T
        if bias is not None:
            h, mag = h + bias.double().cpu(), mag + bias.double().cpu().abs()
        if n < 2:
            h = ACT[activation](h)
    return h, mag


def _random_case(widths, K, A, rows, seed):
    """Default-initialised nn.Linear weights and normal inputs, on the device."""
    torch.manual_seed(seed)
    linears = [torch.nn.Linear(a, b) for a, b in zip((K, *widths), (*widths, A))]
    return torch.randn(rows, K).to(DEV), tuple(t.detach().to(DEV) for m in linears for t in (m.weight, m.bias))


@functools.lru_cache(maxsize=None)
def _integer_case(widths, K, bias3):
    """37 rows, 16 outputs: x and biases integers in [-2, 2], dense weights in {-1, 0, 1}, and the float64 result."""
    g = torch.Generator().manual_seed(1)
    ints = lambda low, high, *shape: torch.randint(low, high + 1, shape, generator=g).float()  # noqa: E731
    (H1, H2), x = widths, ints(-2, 2, 37, K)
    layers = (ints(-1, 1, H1, K), ints(-2, 2, H1), ints(-1, 1, H2, H1), ints(-2, 2, H2), ints(-1, 1, 16, H2), ints(-2, 2, 16) if bias3 else None)
    want, mag = _reference(x, layers, "ReLU")
    assert float(mag.max()) <= 532610 < 2 ** 24  # every partial sum is an integer fp32 holds: any summation order is exact
    return x, layers, want


@pytest.mark.parametrize("K", (1, 3, 6, 20, 64))
@pytest.mark.parametrize("widths", WIDTHS, ids=str)
def test_integer_stacks_equal_float64(widths, K):
    for bias3 in (True, False):
        x, layers, want = _integer_case(widths, K, bias3)
        for rows in (1, 17, 37):
            for A in (1, 5, 16):
                used = tuple(t.to(DEV) for t in layers[:4]) + (layers[4][:A].to(DEV), layers[5][:A].to(DEV) if bias3 else None)
                xs = x[:rows].to(DEV)
                assert ops.mlp2_wave_forward_supported(xs, used, "ReLU")
                before = _launches()
                got = ops.mlp2_wave_forward(xs, used, "ReLU").double().cpu()
                assert _launches() == before + 1
                assert torch.equal(got, want[:rows, :A]), f"{K}->{widths}->{A} at {rows} rows, b3={bias3}: {int((got != want[:rows, :A]).sum())} differ"


@pytest.mark.parametrize("K", (3, 48))
@pytest.mark.parametrize("activation", ("ELU", "Tanh"))
@pytest.mark.parametrize("widths", WIDTHS, ids=str)
def test_random_values_within_four_times_the_library_chains_own_error(widths, activation, K):
    x, layers = _random_case(widths, K, 12, 1000, seed=50)
    chain = F.linear(ACT[activation](F.linear(ACT[activation](F.linear(x, *layers[:2])), *layers[2:4])), *layers[4:])
    want, mag = _reference(x, layers, activation)
    e_kernel, e_chain = (float(((t.double().cpu() - want).abs() / mag).max()) for t in (ops.mlp2_wave_forward(x, layers, activation, 1.0), chain))
    print(f"{activation} {K}->{widths}: kernel {e_kernel:.3e}, library chain {e_chain:.3e} of the accumulated magnitude")
    assert e_chain > 0 and e_kernel <= 4 * e_chain, (e_kernel, e_chain)


def test_rows_do_not_depend_on_tile_wave_or_row_count():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for rows in (16 * 4 * cus - 1, 16 * 4 * cus + 17):   # either side of one grid round
        x, layers = _random_case((64, 64), 6, 5, rows, seed=60)
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(61)).to(DEV)
        out = ops.mlp2_wave_forward(x, layers, "Tanh")
        assert torch.equal(ops.mlp2_wave_forward(x[perm].contiguous(), layers, "Tanh"), out[perm]), rows
        assert torch.equal(ops.mlp2_wave_forward(x[:16].contiguous(), layers, "Tanh"), out[:16]), rows


@pytest.mark.parametrize("widths", ((64, 64), (32, 32)), ids=str)
def test_both_read_paths_give_the_same_bits(widths):
    x, layers = _random_case(widths, 8, 5, 37, seed=65)
    shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(x)   # the same values, 4 bytes off a 16-byte boundary
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and ops.mlp2_wave_forward_supported(shifted, layers, "ELU")
    assert torch.equal(ops.mlp2_wave_forward(shifted, layers, "ELU"), ops.mlp2_wave_forward(x, layers, "ELU"))


@pytest.mark.parametrize("A", (3, 12))
def test_sampling_epilogue_is_normal_sample_logp_behind_the_same_mean(A):
    rows = 16 * 4 * torch.cuda.get_device_properties(0).multi_processor_count + 17
    x, layers = _random_case((64, 64), 3, A, rows, seed=70)
    eps, std = torch.randn(rows, A).to(DEV), (torch.rand(A) * 0.9 + 0.1).to(DEV)
    action, logp, mean, repeated = ops.mlp2_wave_forward(x, layers, "Tanh", std=std, eps=eps)
    assert torch.equal(mean, ops.mlp2_wave_forward(x, layers, "Tanh"))
    want_action, want_logp, want_repeated = ops.normal_sample_logp(mean, std, eps, repeat_std=True)
    assert torch.equal(action, want_action) and torch.equal(logp, want_logp) and torch.equal(repeated, want_repeated)


def _guarded(numel):
    bits = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return bits, bits.data_ptr() + 4 * GUARD


@pytest.mark.parametrize("A", (1, 5, 16))
def test_nothing_outside_the_outputs_is_written_and_refusals_write_nothing(A):
    lib, rows, K = _native.lib(), 37, 6
    x, layers = _random_case((64, 64), K, A, rows, seed=80)
    eps, std = torch.randn(rows, A).to(DEV), (torch.rand(A) * 0.9 + 0.1).to(DEV)
    action, logp, mean, repeated = ops.mlp2_wave_forward(x, layers, "ELU", std=std, eps=eps)

    def call(K, hidden1, code, sampled, out_ptr, bufs=(None, None, None)):
        w1, b1, w2, b2, w3, b3 = (t.data_ptr() for t in layers)
        tail = (std.data_ptr(), eps.data_ptr(), *bufs) if sampled else (None,) * 5
        rc = lib.cusrl_mlp2_wave_forward(x.data_ptr(), rows, K, w1, b1, hidden1, w2, b2, 64, w3, b3, A, code, 1.0, out_ptr, *tail,
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    for sampled in (True, False):
        (out, out_ptr), guarded = _guarded(rows * A), [_guarded(n) for n in (rows * A, rows, rows * A)]
        assert call(K, 64, 2, sampled, out_ptr, tuple(ptr for _, ptr in guarded) if sampled else (None,) * 3) == 0
        for (bits, _), want in [((out, out_ptr), mean)] + (list(zip(guarded, (action, logp, repeated))) if sampled else []):
            assert bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + want.numel():] == SENTINEL).all())
            assert torch.equal(bits[GUARD:GUARD + want.numel()], want.view(torch.int32).flatten())
    # refused by the host entry point, nothing launched: hidden1 = 128, K = 65, an activation code nobody defined
    for k, hidden1, code in ((K, 128, 2), (65, 64, 2), (K, 64, 9)):
        out, out_ptr = _guarded(rows * A)
        assert call(k, hidden1, code, False, out_ptr) == UNSUPPORTED
        assert bool((out == SENTINEL).all())
