"""``cusrl_band_sdpa_fwd_mfma`` on an MI355X against the float64 band formulas of include/cusrl_hip.h (``_causal_attention.band_formulas``),
bound ``BOUND`` of the float64 tensor's largest entry: the 16-query tile's, the 16-key sub-tile's and the d-block's edges, the stride
loop, every side tensor, dead rows, gradients through ``cusrl_band_sdpa_bwd``, row independence, views, guards, refusals and one
module.  Every comparison prints what it measured.

Worst measured on an MI355X over all of it, relative to the largest entry: ``out`` 6.2e-7, ``lse`` 2.9e-7, ``dq`` 4.9e-7, ``dk``
6.8e-7, ``dv`` 3.5e-7; the module's output and gradients inside the context against outside it: 1.7e-7."""

import math

import pytest
import torch

import _causal_attention as _ca
from cusrl_amd import _native

pytestmark = pytest.mark.gpu
DEV, MFMA, VALU, BWD = "cuda:0", "cusrl_band_sdpa_fwd_mfma", "cusrl_band_sdpa_fwd", "cusrl_band_sdpa_bwd"
MID = (2, 2, 33, 17, 20)  # (N, H, Lq, W, D): every axis's edges against this setting; the last shape's 4176 items exceed 4 * 4 * 256
SHAPES = list(dict.fromkeys(
    [MID[:2] + (Lq,) + MID[3:] for Lq in (2, 15, 16, 17, 31, 32, 33, 65)] + [MID[:3] + (W, MID[4]) for W in (1, 15, 16, 17, 31, 32, 33, 48)]
    + [MID[:4] + (D,) for D in (4, 12, 16, 20, 64, 128)] + [(1, 1, 2, 1, 4), (261, 8, 17, 3, 4)]))
CASES = [(shape, option) for shape in SHAPES for option in ("plain", "all")] + [(MID, option) for option in ("valid", "segments", "slopes")]


@pytest.fixture(scope="module")
def ops():
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd.ops


def _counts():
    return tuple(_native.launch_counts.get(symbol, 0) for symbol in (MFMA, VALU, BWD))


def _sides(case):
    return tuple(None if case[name] is None else case[name].to(DEV) for name in ("key_valid", "q_segment", "alibi_slopes"))


def _forward(ops, case, views=None) -> dict:
    q, k, v = views or (case[name].to(DEV) for name in ("q", "k", "v"))
    assert ops.band_sdpa_mfma_supported(q, k, v, case["window"], *_sides(case))
    before = _counts()
    out, lse = ops.band_attention._launch_band_fwd(q, k, v, case["window"], *_sides(case), True)
    assert _counts() == (before[0] + 1, before[1], before[2])
    assert torch.equal(ops.band_sdpa(q, k, v, case["window"], *_sides(case), matrix_core=True), out)
    return {"out": out, "lse": lse}


def _assert_forward_matches(label, got, want, case, dead_rows=()):
    """``lse`` exactly -inf and ``out`` exactly 0 where the float64 row is dead (``dead_rows``: rows that must be), the rest in bound."""
    dead = torch.isinf(want["lse"])  # [N, H, Lq]
    assert dead[..., list(dead_rows)].all() and not (dead_rows and dead.all()) and torch.equal(got["lse"].cpu() == -math.inf, dead)
    assert not got["out"].cpu()[dead.transpose(1, 2)].any()
    alive = lambda lse: torch.where(dead, torch.zeros_like(lse.cpu()), lse.cpu())  # noqa: E731
    _ca.assert_sdpa_matches(label, dict(got, lse=alive(got["lse"])), dict(want, lse=alive(want["lse"])), case, ("out", "lse"))


@pytest.mark.parametrize("shape,option", CASES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_forward_matches_the_float64_formulas(ops, golden, shape, option):
    case = _ca.kernel_case(golden("attention"), shape, option)
    _assert_forward_matches(f"band mfma {shape} {option}", _forward(ops, case), _ca.band_formulas(case), case)


@pytest.mark.parametrize("shape", [(2, 2, 33, 5, 8), (1, 2, 40, 17, 20)], ids=lambda s: "x".join(map(str, s)))
def test_rows_without_a_visible_key(ops, golden, shape):
    """Query rows 0, 15, 16 and the last lose every key of their windows through ``key_valid``: zeros, -inf, nothing NaN."""
    Lq, W = shape[2:4]
    case = _ca.kernel_case(golden("attention"), shape, "slopes")
    case["key_valid"] = torch.ones(shape[0], Lq + W, dtype=torch.bool)
    for row in (rows := [0, 15, 16, Lq - 1]):
        case["key_valid"][:, row:row + W + 1] = False
    _assert_forward_matches(f"band mfma dead rows {shape}", _forward(ops, case), _ca.band_formulas(case), case, rows)


@pytest.mark.parametrize("shape,start", [((2, 2, 33, 17, 24), 0), ((1, 2, 40, 16, 32), 16)])
def test_gradients_through_the_new_forward(ops, golden, shape, start):
    case = _ca.kernel_case(golden("attention"), shape, "all", start)
    q, k, v = (case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v"))
    before = _counts()
    out = ops.band_sdpa(q, k, v, case["window"], *_sides(case), key_grad_from=start, matrix_core=True)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case["dout"].to(DEV))
    assert _counts() == (before[0] + 1, before[1], before[2] + 1) and not dk[:, :start].any() and not dv[:, :start].any()
    got = {"out": out.detach(), "dq": dq, "dk": dk[:, start:], "dv": dv[:, start:]}
    _ca.assert_sdpa_matches(f"band mfma grad {shape} from {start}", got, _ca.band_formulas(case), case)


def test_a_query_rows_bits_are_its_own_and_views_give_the_bits_of_their_copies(ops, golden):
    case = _ca.kernel_case(golden("attention"), (2, 3, 37, 19, 20), "all")
    full, again = _forward(ops, case), _forward(ops, case)
    assert torch.equal(full["out"], again["out"]) and torch.equal(full["lse"], again["lse"])
    alone = dict(case, **{name: case[name][1:2, :, 2:3].contiguous() for name in ("q", "k", "v")}, key_valid=case["key_valid"][1:2],
                 q_segment=case["q_segment"][1:2], alibi_slopes=case["alibi_slopes"][2:3])
    one = _forward(ops, alone)
    assert torch.equal(one["out"][0, :, 0], full["out"][1, :, 2]) and torch.equal(one["lse"][0, 0], full["lse"][1, 2])
    k, v = torch.stack([case["k"], case["v"]], dim=2).to(DEV).unbind(dim=2)  # the slices of a packed [N, Lk, 2, H, D] projection
    q = case["q"].to(DEV).transpose(0, 1).contiguous().transpose(0, 1)  # the [L, N, H, D] memory of a sequence-first module
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    views = _forward(ops, case, (q, k, v))
    assert torch.equal(views["out"], full["out"]) and torch.equal(views["lse"], full["lse"])


def _raw(case, shift=0):
    # the raw entry on 12345-filled out / lse with 64 guard floats on both sides, q `shift` floats into its buffer
    N, Lq, H, D = case["q"].shape
    Lk = case["k"].shape[1]
    q = torch.zeros(case["q"].numel() + 4, device=DEV)[shift:shift + case["q"].numel()].copy_(case["q"].flatten())
    k, v, sides = case["k"].to(DEV), case["v"].to(DEV), _sides(case)
    out, lse = (torch.full((128 + numel,), 12345.0, device=DEV) for numel in (N * Lq * H * D, N * H * Lq))
    status = _native.lib().cusrl_band_sdpa_fwd_mfma(q.data_ptr(), Lq * H * D, H * D, k.data_ptr(), Lk * H * D, H * D, v.data_ptr(), Lk * H * D, H * D,
                                                    *(None if side is None else side.data_ptr() for side in sides), 1.0 / math.sqrt(D),
                                                    out[64:].data_ptr(), lse[64:].data_ptr(), N, H, Lq, case["window"], D,
                                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, out, lse


def test_the_launch_stays_inside_out_and_lse_and_refusals_write_nothing(ops, golden):
    g = golden("attention")
    for shape in ((2, 3, 33, 17, 8), (1, 2, 17, 16, 128)):
        case = _ca.kernel_case(g, shape, "all")
        (status, out, lse), want = _raw(case), _forward(ops, case)
        assert status == 0
        for buffer, tensor in ((out, want["out"]), (lse, want["lse"])):
            assert (buffer[:64] == 12345.0).all() and (buffer[-64:] == 12345.0).all() and torch.equal(buffer[64:-64], tensor.flatten())
    odd, fine, step = (_ca.kernel_case(g, shape, "all") for shape in ((2, 3, 5, 7, 6), (2, 3, 5, 7, 8), (2, 3, 1, 7, 8)))
    for case, shift in ((odd, 0), (fine, 1), (step, 0)):
        status, out, lse = _raw(case, shift)
        assert status == _native._CONSTANTS["E_UNSUPPORTED"] and (out == 12345.0).all() and (lse == 12345.0).all()
        q, k, v = (case[name].to(DEV) for name in ("q", "k", "v"))
        if shift:
            q = torch.zeros(q.numel() + 4, device=DEV)[shift:shift + q.numel()].copy_(q.flatten()).view(q.shape)
        before = _counts()
        assert ops.band_sdpa_supported(q, k, v, 7, *_sides(case)) and not ops.band_sdpa_mfma_supported(q, k, v, 7, *_sides(case))
        assert torch.equal(ops.band_sdpa(q, k, v, 7, *_sides(case), matrix_core=True), ops.band_sdpa(q, k, v, 7, *_sides(case)))
        assert _counts() == (before[0], before[1] + 2, before[2])


def test_a_causal_module_reaches_the_kernel_through_the_context(ops):
    import cusrl_amd as cusrl

    torch.manual_seed(11)
    module = cusrl.nn.CausalMultiheadSelfAttention(embed_dim=32, num_heads=2, window_size=4).to(DEV)
    x, done = torch.randn(6, 2, 32, device=DEV), torch.zeros(6, 2, 1, dtype=torch.bool, device=DEV)
    done[2, 0] = done[4, 1] = True
    with torch.no_grad():
        _, memory = module(torch.randn(3, 2, 32, device=DEV), None)

    def run():
        leaf = x.clone().requires_grad_(True)
        out, _ = module(leaf, memory, done=done)
        return [out.detach(), *torch.autograd.grad(out.sum(), [leaf, *module.parameters()])]

    before = _counts()
    outside = run()
    assert _counts() == (before[0], before[1] + 1, before[2] + 1), "nothing is routed to the MFMA forward by default"
    with ops.matrix_core_attention():
        inside = run()
    assert _counts() == (before[0] + 1, before[1] + 1, before[2] + 2)
    errors = [_ca.relative_to_largest(a, b) for a, b in zip(inside, outside)]
    print(f"causal module inside the context against outside it: worst {max(errors):.3e} of the largest entry")
    assert max(errors) <= _ca.BOUND, errors
