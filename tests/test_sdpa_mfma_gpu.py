"""``cusrl_sdpa_fwd_mfma`` on an MI355X against the float64 formulas of include/cusrl_hip.h (``_attention.sdpa_formulas``), bound
``_attention.BOUND`` of the float64 tensor's largest entry: the wave's, workgroup's, key tile's and d-block's edges, masks in every
form with fully masked rows, gradients through ``cusrl_sdpa_bwd``, row independence, views, guards, refusals and one module.
Every comparison prints what it measured.

Worst measured on an MI355X over all of it, relative to the largest entry: ``out`` 6.7e-7, ``lse`` 2.2e-7, ``dq`` 9.7e-7, ``dk``
1.06e-6, ``dv`` 7.3e-7; the module's output and gradients inside the context against outside it: 1.2e-7."""

import math

import pytest
import torch

import _attention
from cusrl_amd import _native

pytestmark = pytest.mark.gpu
DEV, MFMA, VALU = "cuda:0", "cusrl_sdpa_fwd_mfma", "cusrl_sdpa_fwd"
MID = (1, 2, 33, 47, 20)  # (N, H, Lq, Lk, D): every axis's edges against this setting; the last case strides over 1032 work items
SHAPES = list(dict.fromkeys(
    [MID[:2] + (Lq,) + MID[3:] for Lq in (1, 15, 16, 17, 63, 64, 65)] + [MID[:3] + (Lk, MID[4]) for Lk in (1, 31, 32, 33, 65)]
    + [MID[:4] + (D,) for D in (4, 12, 16, 20, 64, 128)] + [(1, 1) + MID[2:], (2, 3) + MID[2:], (2, 3, 65, 65, 20), (1, 1, 65, 33, 128),
                                                             (129, 8, 3, 5, 4)]))
MASK_FORMS = {"LL": lambda N, H, Lq, Lk: (Lq, Lk), "N1LL": lambda N, H, Lq, Lk: (N, 1, Lq, Lk), "NHLL": lambda N, H, Lq, Lk: (N, H, Lq, Lk)}


@pytest.fixture(scope="module")
def ops():
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd.ops


def _count(symbol):
    return _native.launch_counts.get(symbol, 0)


def _forward(ops, case, views=None) -> dict:
    """``out`` and ``lse`` of one ``cusrl_sdpa_fwd_mfma`` launch on the case's operands (``views``: device views in their place)."""
    mask = None if case["mask"] is None else case["mask"].to(DEV)
    q, k, v = views or (case[name].to(DEV) for name in ("q", "k", "v"))
    assert ops.sdpa_mfma_supported(q, k, v, mask, 0.0, case["is_causal"])
    before = _count(MFMA), _count(VALU)
    out, lse = ops.attention._launch_sdpa_fwd(q, k, v, mask, case["is_causal"], True)
    assert (_count(MFMA), _count(VALU)) == (before[0] + 1, before[1])
    assert torch.equal(ops.sdpa(q, k, v, attn_mask=mask, is_causal=case["is_causal"], matrix_core=True), out)
    return {"out": out, "lse": lse}


@pytest.mark.parametrize("mask", [None, "causal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_the_float64_formulas(ops, golden, shape, mask):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    _attention.assert_sdpa_matches(f"mfma {shape} {mask}", _forward(ops, case), _attention.sdpa_formulas(case), case, ("out", "lse"))


@pytest.mark.parametrize("form", [*MASK_FORMS, "transposed"])
@pytest.mark.parametrize("kind", ["bool", "float"])
@pytest.mark.parametrize("shape", [(2, 2, 33, 47, 8), (1, 2, 65, 33, 16)], ids=lambda s: "x".join(map(str, s)))
def test_masks_and_fully_masked_rows(ops, golden, shape, kind, form):
    """Fully masked query rows at the first row, across a wave's edge and at the last row: ``out`` exactly 0 and ``lse`` exactly
    -inf there, nothing NaN (``assert_sdpa_matches``), every other row in bound."""
    N, H, Lq, Lk, _ = shape
    rows = [0, 15, 16, Lq - 1]
    if form == "transposed":
        case = _attention.kernel_case(golden("attention"), shape, kind, (N, H, Lk, Lq))
        case["mask"] = case["mask"].transpose(-1, -2)
        case["mask"][..., rows, :] = False if kind == "bool" else -math.inf
        assert not case["mask"].is_contiguous()
    else:
        case = _attention.kernel_case(golden("attention"), shape, kind, MASK_FORMS[form](N, H, Lq, Lk), masked_rows=rows)
    got, want = _forward(ops, case), _attention.sdpa_formulas(case)
    dead = torch.isinf(want["lse"])
    assert dead[..., rows].all() and not dead.all() and torch.equal(got["lse"].cpu() == -math.inf, dead) and not got["out"][:, rows].any()
    alive = lambda lse: torch.where(dead, torch.zeros_like(lse.cpu()), lse.cpu())  # noqa: E731
    _attention.assert_sdpa_matches(f"mfma {shape} {kind} {form}", dict(got, lse=alive(got["lse"])), dict(want, lse=alive(want["lse"])), case, ("out", "lse"))


@pytest.mark.parametrize("shape,mask", [((2, 2, 33, 33, 24), "causal"), ((1, 2, 65, 130, 32), "bool")])
def test_gradients_through_the_new_forward(ops, golden, shape, mask):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    q, k, v = (case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v"))
    before = _count(MFMA), _count(VALU), _count("cusrl_sdpa_bwd")
    out = ops.sdpa(q, k, v, attn_mask=None if case["mask"] is None else case["mask"].to(DEV), is_causal=case["is_causal"], matrix_core=True)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case["dout"].to(DEV))
    assert (_count(MFMA), _count(VALU), _count("cusrl_sdpa_bwd")) == (before[0] + 1, before[1], before[2] + 1)
    _attention.assert_sdpa_matches(f"mfma grad {shape}", {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}, _attention.sdpa_formulas(case), case)


def test_a_query_rows_bits_are_its_own(ops, golden):
    case = _attention.kernel_case(golden("attention"), (2, 3, 65, 47, 20), "float")
    full, again = _forward(ops, case), _forward(ops, case)
    assert torch.equal(full["out"], again["out"]) and torch.equal(full["lse"], again["lse"])
    alone = {"q": case["q"][1:2, 37:38, 2:3].contiguous(), "k": case["k"][1:2, :, 2:3].contiguous(), "v": case["v"][1:2, :, 2:3].contiguous(),
             "mask": case["mask"][1:2, 2:3, 37:38].contiguous(), "is_causal": False}
    one = _forward(ops, alone)
    assert torch.equal(one["out"][0, 0, 0], full["out"][1, 37, 2]) and torch.equal(one["lse"][0, 0, 0], full["lse"][1, 2, 37])


def test_packed_and_transposed_views_give_the_bits_of_their_copies(ops, golden):
    case = _attention.kernel_case(golden("attention"), (2, 3, 19, 19, 8), "causal")
    plain = _forward(ops, case)
    q, k, v = torch.stack([case["q"], case["k"], case["v"]], dim=2).to(DEV).unbind(dim=2)  # the slices of [N, L, 3, H, D]
    first = tuple(case[name].to(DEV).transpose(0, 1).contiguous().transpose(0, 1) for name in ("q", "k", "v"))  # batch_first=False
    for views in ((q, k, v), first):
        assert not views[0].is_contiguous()
        got = _forward(ops, case, views)
        assert torch.equal(got["out"], plain["out"]) and torch.equal(got["lse"], plain["lse"])


def _raw(case, shift=0, keep_and_bias=False):
    """The raw entry on 12345-filled ``out`` / ``lse`` with 64 guard floats on both sides, ``q`` ``shift`` floats into its buffer."""
    N, Lq, H, D = case["q"].shape
    Lk = case["k"].shape[1]
    q = torch.zeros(case["q"].numel() + 4, device=DEV)[shift:shift + case["q"].numel()].copy_(case["q"].flatten())
    k, v = case["k"].to(DEV), case["v"].to(DEV)
    out, lse = (torch.full((128 + numel,), 12345.0, device=DEV) for numel in (N * Lq * H * D, N * H * Lq))
    mask = torch.ones(Lq, Lk, device=DEV).data_ptr() if keep_and_bias else None  # (handed in as keep-mask AND bias: refused unread)
    status = _native.lib().cusrl_sdpa_fwd_mfma(q.data_ptr(), Lq * H * D, H * D, k.data_ptr(), Lk * H * D, H * D, v.data_ptr(), Lk * H * D, H * D,
                                               mask, mask, 0, 0, 0, 0, int(case["is_causal"]), 1.0 / math.sqrt(D), out[64:].data_ptr(),
                                               lse[64:].data_ptr(), N, H, Lq, Lk, D, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, out, lse


@pytest.mark.parametrize("shape,mask", [((2, 3, 33, 47, 8), "causal"), ((1, 2, 17, 16, 128), None)])
def test_the_launch_stays_inside_out_and_lse(ops, golden, shape, mask):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    status, out, lse = _raw(case)
    want = _forward(ops, case)
    assert status == 0
    for buffer, tensor in ((out, want["out"]), (lse, want["lse"])):
        assert (buffer[:64] == 12345.0).all() and (buffer[-64:] == 12345.0).all() and torch.equal(buffer[64:-64], tensor.flatten())


def test_refusals_write_nothing_and_fall_through(ops, golden):
    g = golden("attention")
    odd, fine = _attention.kernel_case(g, (2, 3, 5, 7, 6)), _attention.kernel_case(g, (2, 3, 5, 7, 8))
    for case, kwargs, code in ((odd, {}, "E_UNSUPPORTED"), (fine, {"shift": 1}, "E_UNSUPPORTED"), (fine, {"keep_and_bias": True}, "E_INVALID")):
        status, out, lse = _raw(case, **kwargs)
        assert status == _native._CONSTANTS[code] and (out == 12345.0).all() and (lse == 12345.0).all()
    q, k, v = (odd[name].to(DEV) for name in ("q", "k", "v"))
    before = _count(MFMA)
    assert not ops.sdpa_mfma_supported(q, k, v) and torch.equal(ops.sdpa(q, k, v, matrix_core=True), ops.sdpa(q, k, v))
    shifted = torch.zeros(q.numel() + 4, device=DEV)[1:1 + q.numel()].view(q.shape)
    assert ops.sdpa_supported(shifted, k, v) and not ops.sdpa_mfma_supported(shifted, k, v) and _count(MFMA) == before


def test_a_module_reaches_the_kernel_through_the_context(ops):
    import cusrl_amd as cusrl

    torch.manual_seed(11)
    module = cusrl.MultiheadSelfAttention(embed_dim=32, num_heads=2).to(DEV)
    x = torch.randn(2, 40, 32, device=DEV)

    def run():
        leaf = x.clone().requires_grad_(True)
        out = module(leaf, is_causal=True)
        return [out.detach(), *torch.autograd.grad(out.sum(), [leaf, *module.parameters()])]

    before = _count(MFMA), _count(VALU)
    outside = run()
    with ops.matrix_core_attention(False):
        assert torch.equal(run()[0], outside[0])
    assert (_count(MFMA), _count(VALU)) == (before[0], before[1] + 2), "nothing is routed to the MFMA forward by default"
    with ops.matrix_core_attention():
        inside = run()
    assert (_count(MFMA), _count(VALU)) == (before[0] + 1, before[1] + 2)
    errors = [_attention.relative_to_largest(a, b) for a, b in zip(inside, outside)]
    print(f"module inside the context against outside it: worst {max(errors):.3e} of the largest entry")
    assert max(errors) <= _attention.BOUND, errors
