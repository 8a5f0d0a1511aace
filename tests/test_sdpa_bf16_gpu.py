"""``cusrl_sdpa_fwd_bf16`` on an MI355X against the float64 formulas of include/cusrl_hip.h (``_attention.sdpa_formulas``) on the
bf16-rounded operands.  Bounds, derived: ``lse`` within ``_attention.BOUND`` of its largest entry (the products of two bf16 are exact
in fp32); per element ``|out - ref| <= 2^-8 (sum_j p_ij |v_jhd| + |ref_ihd|) + 1e-5 max|v|``: the rounding of P to bf16, that of
``out`` to bf16, the standing fp32 bound.  Prints the worst ratio of error to bound (0.751 over all of it on an MI355X)."""

import math

import pytest
import torch

import _attention
import cusrl_amd as cusrl
from cusrl_amd import _native, ops

pytestmark = pytest.mark.gpu
DEV, BF16, BWD = "cuda:0", "cusrl_sdpa_fwd_bf16", "cusrl_sdpa_bwd"
MID = (1, 2, 33, 47, 24)  # (N, H, Lq, Lk, D): every axis's edges against this setting; the last shape strides over 1032 work items
SHAPES = list(dict.fromkeys(
    [MID[:2] + (Lq,) + MID[3:] for Lq in (1, 15, 16, 17, 63, 64, 65)] + [MID[:3] + (Lk, MID[4]) for Lk in (1, 31, 32, 33, 65)]
    + [MID[:4] + (D,) for D in (8, 16, 24, 32, 40, 64, 128)] + [(2, 3, 65, 65, 24), (1, 1, 65, 33, 128), (129, 8, 3, 5, 8)]))


def _count(*symbols):
    return tuple(_native.launch_counts.get(symbol, 0) for symbol in symbols)


def _case(golden, shape, mask=None, **kwargs) -> dict:
    """The kernel case with ``q``, ``k``, ``v`` and ``dout`` rounded to bf16 (kept as fp32: what the float64 formulas read)."""
    case = _attention.kernel_case(golden("attention"), shape, mask, **kwargs)
    return dict(case, **{name: case[name].bfloat16().float() for name in ("q", "k", "v", "dout")})


def _forward(case, views=None) -> dict:
    mask = None if case["mask"] is None else case["mask"].to(DEV)
    q, k, v = views or (case[name].to(DEV).bfloat16() for name in ("q", "k", "v"))
    assert ops.sdpa_bf16_supported(q, k, v, mask, 0.0, case["is_causal"])
    before = _count(BF16)
    out, lse = ops.attention._launch_sdpa_fwd_bf16(q, k, v, mask, case["is_causal"])
    assert _count(BF16) == (before[0] + 1,) and out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert torch.equal(ops.sdpa(q, k, v, attn_mask=mask, is_causal=case["is_causal"], matrix_core=True), out)
    return {"out": out, "lse": lse}


def _assert_in_bound(label, got, case):
    want, weight = _attention.sdpa_formulas(case), _attention.sdpa_formulas(dict(case, v=case["v"].abs()))["out"]  # sum_j p_ij |v_j|
    out, lse, dead = got["out"].cpu().double(), got["lse"].cpu().double(), torch.isinf(want["lse"])
    assert not torch.isnan(out).any() and torch.equal(lse == -math.inf, dead) and not out[dead.transpose(1, 2)].any()
    bound = 2.0 ** -8 * (weight + want["out"].abs()) + 1e-5 * case["v"].abs().max()
    ratio = float(((out - want["out"]).abs() / bound).max())
    error = _attention.relative_to_largest(lse.masked_fill(dead, 0.0), want["lse"].masked_fill(dead, 0.0))
    print(f"{label}: out at {ratio:.3f} of its bound, lse {error:.3e} of the largest entry")
    assert ratio <= 1.0 and error <= _attention.BOUND


@pytest.mark.parametrize("mask", [None, "causal"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_is_inside_the_derived_bounds(golden, shape, mask):
    case = _case(golden, shape, mask)
    got = _forward(case)
    _assert_in_bound(f"bf16 {shape} {mask}", got, case)
    if shape[3] == 1:  # one key: every row is that key's value, exactly
        assert torch.equal(got["out"], case["v"].to(DEV).bfloat16().expand_as(got["out"]))


@pytest.mark.parametrize("form", ["LL", "NHLL"])
@pytest.mark.parametrize("kind", ["bool", "float"])
@pytest.mark.parametrize("shape", [(2, 2, 33, 47, 8), (1, 2, 65, 33, 16)], ids=str)
def test_masks_and_fully_masked_rows(golden, shape, kind, form):
    (N, H, Lq, Lk, _), rows = shape, [0, 15, 16, shape[2] - 1]  # fully masked: the first row, a wave's edge, the last row
    case = _case(golden, shape, kind, mask_shape=(Lq, Lk) if form == "LL" else (N, H, Lq, Lk), masked_rows=rows)
    got = _forward(case)
    assert (got["lse"][..., rows] == -math.inf).all() and not (got["lse"] == -math.inf).all()
    _assert_in_bound(f"bf16 {shape} {kind} {form}", got, case)  # (also: out exactly 0 and lse exactly -inf there, nothing NaN)


def test_a_query_rows_bits_are_its_own_and_views_give_the_bits_of_their_copies(golden):
    case = _case(golden, (2, 3, 65, 47, 24), "float")
    full, again = _forward(case), _forward(case)
    assert torch.equal(full["out"], again["out"]) and torch.equal(full["lse"], again["lse"])
    alone = {"q": case["q"][1:2, 37:38, 2:3].contiguous(), "k": case["k"][1:2, :, 2:3].contiguous(), "v": case["v"][1:2, :, 2:3].contiguous(),
             "mask": case["mask"][1:2, 2:3, 37:38].contiguous(), "is_causal": False}
    one = _forward(alone)
    assert torch.equal(one["out"][0, 0, 0], full["out"][1, 37, 2]) and torch.equal(one["lse"][0, 0, 0], full["lse"][1, 2, 37])
    case = _case(golden, (2, 3, 19, 19, 8), "causal")
    plain = _forward(case)
    views = torch.stack([case["q"], case["k"], case["v"]], dim=2).to(DEV).bfloat16().unbind(dim=2)  # the slices of [N, L, 3, H, D]
    packed = _forward(case, views)
    assert torch.equal(packed["out"], plain["out"]) and torch.equal(packed["lse"], plain["lse"])


def test_refusals_write_nothing_and_count_no_launch(golden):
    for N, H, Lq, Lk, D, shift in ((2, 3, 5, 7, 12, 0), (2, 3, 5, 7, 8, 1)):  # a head size outside the set; q one element into its buffer
        case = _case(golden, (N, H, Lq, Lk, D))
        q = torch.zeros(N * Lq * H * D + 8, device=DEV, dtype=torch.bfloat16)[shift:shift + N * Lq * H * D].view(N, Lq, H, D).copy_(case["q"])
        k, v = case["k"].to(DEV).bfloat16(), case["v"].to(DEV).bfloat16()
        out, lse = torch.full((N * Lq * H * D,), 12345.0, device=DEV, dtype=torch.bfloat16), torch.full((N * H * Lq,), 12345.0, device=DEV)
        status = _native.lib().cusrl_sdpa_fwd_bf16(q.data_ptr(), Lq * H * D, H * D, k.data_ptr(), Lk * H * D, H * D, v.data_ptr(), Lk * H * D, H * D,
                                                   None, None, 0, 0, 0, 0, 0, 1.0 / math.sqrt(D), out.data_ptr(), lse.data_ptr(), N, H, Lq, Lk, D,
                                                   torch.cuda.current_stream().cuda_stream)
        before = _count(BF16)  # (the comparisons below synchronise)
        assert status == _native._CONSTANTS["E_UNSUPPORTED"] and (out == 12345.0).all() and (lse == 12345.0).all()
        assert not ops.sdpa_bf16_supported(q, k, v) and (shift or ops.sdpa(q, k, v, matrix_core=True).dtype == torch.bfloat16) and _count(BF16) == before


@pytest.mark.parametrize("mask", [None, "causal"])
@pytest.mark.parametrize("shape", [(2, 2, 33, 47, 24), (1, 2, 65, 33, 64)], ids=str)
def test_gradients_against_torchs_bf16_attention_as_the_yardstick(golden, shape, mask):
    """No derived bound: per tensor at most twice the error of ``F.scaled_dot_product_attention`` on the same bf16 leaves."""
    case = _case(golden, shape, mask)
    want, dout, before = _attention.sdpa_formulas(case), case["dout"].to(DEV).bfloat16(), _count(BF16, BWD)
    q, k, v = (case[name].to(DEV).bfloat16().requires_grad_(True) for name in ("q", "k", "v"))
    mine = torch.autograd.grad(ops.sdpa(q, k, v, is_causal=case["is_causal"], matrix_core=True), (q, k, v), dout)
    assert _count(BF16, BWD) == (before[0] + 1, before[1] + 1) and all(g.dtype == torch.bfloat16 for g in mine)
    torchs = torch.autograd.grad(ops.attention._sdpa_expression(q, k, v, None, 0.0, case["is_causal"]), (q, k, v), dout)
    for name, a, b in zip(("dq", "dk", "dv"), mine, torchs):
        new, yardstick = _attention.relative_to_largest(a.float(), want[name]), _attention.relative_to_largest(b.float(), want[name])
        print(f"bf16 grad {shape} {mask} {name}: {new:.3e} of the largest entry, torch's {yardstick:.3e}")
        assert new <= 2 * yardstick, (name, new, yardstick)


def test_a_module_under_autocast_reaches_the_kernel_through_the_context():
    """Inside against outside: each attention output is within 2^-8 (sum p |v| + |out|) <= 2^-7 max|v| of the exact one and ``out_proj``
    rounds once more, so 2^-6 of the largest entry bounds their distance if the projection does not amplify a relative error."""
    torch.manual_seed(11)
    module, x, before = cusrl.MultiheadSelfAttention(embed_dim=32, num_heads=2).to(DEV), torch.randn(2, 40, 32, device=DEV), _count(BF16)
    with torch.autocast("cuda", torch.bfloat16):
        outside = module(x, is_causal=True)
        assert _count(BF16) == before, "nothing is routed to the bf16 forward by default"
        with ops.matrix_core_attention():
            inside = module(x, is_causal=True)
    assert _count(BF16) == (before[0] + 1,) and inside.dtype == outside.dtype == torch.bfloat16
    error = _attention.relative_to_largest(inside.float(), outside.float())
    print(f"module inside the context against outside it: {error:.3e} of the largest entry")
    assert error <= 2.0 ** -6
