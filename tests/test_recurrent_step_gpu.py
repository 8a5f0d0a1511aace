"""``cusrl_gru_step_forward`` / ``cusrl_lstm_step_forward`` (csrc/recurrent_step.hip) on an MI355X against ``torch.nn.GRU`` /
``torch.nn.LSTM`` in float64: within four times the per-step chain's own error, rows independent of the work split, the same bits
from both read paths and from in-place layer slices, guarded, and reached from ``nn.Gru`` / ``nn.Lstm`` inside
``ops.fused_recurrent_step()``."""

from __future__ import annotations

import copy

import pytest
import torch

from cusrl_amd import _native, nn, ops
from cusrl_amd.nn.gru import gru_forward, lstm_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELLS = ("GRU", "LSTM")
SYMBOL = {"GRU": "cusrl_gru_step_forward", "LSTM": "cusrl_lstm_step_forward"}
UNSUPPORTED = -3                   # CUSRL_E_UNSUPPORTED
GUARD, SENTINEL = 64, 0x7FA5A5A5   # floats on either side of a guarded output, and the bits they hold


def _launches() -> int:
    return sum(_native.launch_counts.get(symbol, 0) for symbol in SYMBOL.values())


def _case(cell, I, H, bias, B, seed):
    """A default-initialised CPU ``torch.nn`` module, normal x and 0.5 * normal states on the device."""
    torch.manual_seed(seed)
    module = getattr(torch.nn, cell)(I, H, bias=bias)
    return module, torch.randn(B, I).to(DEV), tuple((0.5 * torch.randn(B, H)).to(DEV) for _ in range(1 if cell == "GRU" else 2))


def _params(module, layer=0):
    names = (f"weight_ih_l{layer}", f"weight_hh_l{layer}", f"bias_ih_l{layer}", f"bias_hh_l{layer}")
    return tuple(getattr(module, name).detach().to(DEV) if module.bias or "weight" in name else None for name in names)


def _step(cell, x, states, params, out=None):
    if cell == "GRU":
        return (ops.gru_step_forward(x, *states, *params, out=None if out is None else out[0]),)
    return ops.lstm_step_forward(x, *states, *params, out=out)


def _module_states(cell, states):
    return states[0][None] if cell == "GRU" else tuple(s[None] for s in states)


def _float64(cell, module, x, states):
    with torch.no_grad():
        _, last = copy.deepcopy(module).double()(x.double().cpu()[None], _module_states(cell, tuple(s.double().cpu() for s in states)))
    return (last[0],) if cell == "GRU" else (last[0][0], last[1][0])


def _error(got, want) -> float:
    return max(float((g.double().cpu() - w).abs().max()) for g, w in zip(got, want))


@pytest.mark.parametrize("bias", (True, False))
@pytest.mark.parametrize("I", (1, 3, 20, 256))
@pytest.mark.parametrize("H", (16, 48, 256))
@pytest.mark.parametrize("cell", CELLS)
def test_values_within_four_times_the_chains_own_error(cell, H, I, bias):
    """Worst pairs measured (kernel, chain): see DESIGN.md §7 "Recurrent step on the matrix cores"."""
    module, x, states = _case(cell, I, H, bias, 273, seed=10)
    want = _float64(cell, module, x, states)
    before = _native.launch_counts.get(SYMBOL[cell], 0)
    got = _step(cell, x, states, _params(module))
    assert _native.launch_counts.get(SYMBOL[cell], 0) == before + 1
    with torch.no_grad():
        _, last = (gru_forward if cell == "GRU" else lstm_forward)(copy.deepcopy(module).to(DEV), x[None], _module_states(cell, states))
    e_kernel, e_chain = _error(got, want), _error((last[0],) if cell == "GRU" else (last[0][0], last[1][0]), want)
    print(f"{cell} I={I} H={H} bias={bias}: kernel {e_kernel:.3e}, chain {e_chain:.3e}")
    assert e_chain > 0 and e_kernel <= 4 * e_chain, (e_kernel, e_chain)


@pytest.mark.parametrize("cell", CELLS)
def test_rows_do_not_depend_on_the_split(cell):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (16 * 4 * cus - 17, 16 * 4 * cus + 17):   # either side of one grid round: two slices, one slice
        module, x, states = _case(cell, 6, 48, True, B, seed=20)
        params = _params(module)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(21)).to(DEV)
        out = _step(cell, x, states, params)
        for got, want in zip(_step(cell, x[perm].contiguous(), tuple(s[perm].contiguous() for s in states), params), out):
            assert torch.equal(got, want[perm]), B
        for rows in (16, 1):   # (three slices)
            for got, want in zip(_step(cell, x[:rows].contiguous(), tuple(s[:rows].contiguous() for s in states), params), out):
                assert torch.equal(got, want[:rows]), (B, rows)


@pytest.mark.parametrize("cell", CELLS)
def test_both_read_paths_give_the_same_bits(cell):
    module, x, states = _case(cell, 8, 32, True, 37, seed=30)
    shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(x)   # the same values, 4 bytes off a 16-byte boundary
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    for got, want in zip(_step(cell, shifted, states, _params(module)), _step(cell, x, states, _params(module))):
        assert torch.equal(got, want)


def _guarded(numel):
    bits = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return bits, bits[GUARD:GUARD + numel].view(torch.float32)


@pytest.mark.parametrize("cell", CELLS)
def test_layer_slices_in_place_and_refusals_write_nothing(cell):
    B, I, H = 37, 6, 16
    module, x, states = _case(cell, I, H, True, B, seed=40)
    params = _params(module)
    want = _step(cell, x, states, params)
    # layer 1's slices of [B, 2H] matrices, in and out
    wide = tuple(torch.randn(B, 2 * H, device=DEV) for _ in states)
    for w, s in zip(wide, states):
        w[:, H:] = s
    guarded = [_guarded(B * 2 * H) for _ in states]
    _step(cell, x, tuple(w[:, H:] for w in wide), params, out=tuple(flat.view(B, 2 * H)[:, H:] for _, flat in guarded))
    for (bits, flat), expected in zip(guarded, want):
        assert torch.equal(flat.view(B, 2 * H)[:, H:], expected)
        assert bool((flat.view(torch.int32).view(B, 2 * H)[:, :H] == SENTINEL).all())
        assert bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[-GUARD:] == SENTINEL).all())

    def refused(I=I, H=H, alias=False, params=params):
        outs = [_guarded(B * 16)[1] for _ in states]
        ins = outs if alias else states
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rc = getattr(_native.lib(), SYMBOL[cell])(x.data_ptr(), B, I, *map(ptr, ins), H, *map(ptr, params), H, *map(ptr, outs), H,
                                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc == UNSUPPORTED and all(bool((o.view(torch.int32) == SENTINEL).all()) for o in outs)

    assert refused(H=24) and refused(H=272) and refused(I=257) and refused(alias=True) and refused(params=(*params[:3], None))


@pytest.mark.parametrize("cell", CELLS)
def test_modules_take_the_kernel_inside_the_context_only(cell):
    torch.manual_seed(50)
    module = (nn.Gru if cell == "GRU" else nn.Lstm)(6, 32, num_layers=2).to(DEV)
    x, memory = torch.randn(1, 37, 6, device=DEV), torch.randn(37, 64, device=DEV) * 0.5
    memory = memory if cell == "GRU" else {"hidden": memory, "cell": torch.randn(37, 64, device=DEV) * 0.5}
    flat = lambda result: (result[0], *((result[1],) if cell == "GRU" else (result[1]["hidden"], result[1]["cell"])))  # noqa: E731
    with torch.no_grad():
        outside, before = flat(module.rnn(x, memory)), _launches()
        with ops.fused_recurrent_step():
            inside = flat(module.rnn(x, memory))
        assert _launches() == before + 2
        reference = copy.deepcopy(module.rnn).cpu().double()
        state = memory.cpu().double() if cell == "GRU" else {k: v.cpu().double() for k, v in memory.items()}
        want = flat(torch.nn.Module.__call__(reference, x.cpu().double(), state))
    for got, chain, exact in zip(inside, outside, want):
        assert got.shape == chain.shape and (got.dim() == 3 or got.stride() == chain.stride())
        own = float((chain.double().cpu() - exact).abs().max())
        assert own > 0 and float((got.double().cpu() - exact).abs().max()) <= 4 * own
    with ops.fused_recurrent_step():
        before = _launches()
        with torch.no_grad():
            long = torch.randn(3, 37, 6, device=DEV)
            assert all(torch.equal(a, b) for a, b in zip(flat(module.rnn(long, memory)), flat(_outside(module, long, memory))))
        assert all(torch.equal(a, b) for a, b in zip(flat(module.rnn(x, memory)), outside))   # grad enabled: parameters require it
        assert _launches() == before


def _outside(module, x, memory):
    with ops.fused_recurrent_step(False), torch.no_grad():
        return module.rnn(x, memory)
