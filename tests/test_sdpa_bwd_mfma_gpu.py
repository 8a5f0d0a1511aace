"""``cusrl_sdpa_bwd_mfma`` on an MI355X against the float64 formulas of include/cusrl_hip.h (``_attention.sdpa_formulas``), bound
``_attention.BOUND`` of the float64 tensor's largest entry, on ``out`` / ``lse`` of ``cusrl_sdpa_fwd``: the edges of the wave, the
streamed tile, the workgroup and the d-block in both passes, masks in every form, the autograd routes, row independence, views,
guards and refusals.  Every comparison prints what it measured.  Worst measured on an MI355X over all of it, relative to the largest
entry: ``dq`` 1.16e-6, ``dk`` 9.8e-7, ``dv`` 8.7e-7; the module inside the context against outside it: 1.9e-7."""

import math

import pytest
import torch

import _attention
from cusrl_amd import _native

pytestmark = pytest.mark.gpu
DEV, MFMA, VALU = "cuda:0", "cusrl_sdpa_bwd_mfma", "cusrl_sdpa_bwd"
MID = (1, 2, 33, 47, 20)  # (N, H, Lq, Lk, D): every axis's edges against this setting; the last case takes two rounds of the item order
EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)  # the wave, the streamed tile and the workgroup (causal: Lq > Lk and Lq < Lk among them)
SHAPES = list(dict.fromkeys([MID[:2] + (Lq,) + MID[3:] for Lq in EDGES] + [MID[:3] + (Lk, MID[4]) for Lk in EDGES]
                            + [MID[:4] + (D,) for D in (4, 12, 16, 20, 64, 128)] + [(65, 8, 65, 65, 4)]))


@pytest.fixture(scope="module")
def ops():
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd.ops


def _counts(*symbols):
    return tuple(_native.launch_counts.get(symbol, 0) for symbol in symbols)


def _device(case, ops):
    """The case's operands on the device with ``out`` / ``lse`` of one ``cusrl_sdpa_fwd`` launch."""
    on = {name: None if case[name] is None else case[name].to(DEV) for name in ("q", "k", "v", "dout", "mask")}
    on["out"], on["lse"] = ops.attention._launch_sdpa_fwd(on["q"], on["k"], on["v"], on["mask"], case["is_causal"], False)
    return on


def _backward(ops, case, **views) -> dict:
    """``dq``, ``dk``, ``dv`` of one ``cusrl_sdpa_bwd_mfma`` call (``views``: device tensors in the operands' place)."""
    on = {**_device(case, ops), **views}
    before = _counts(MFMA, VALU)
    grads = ops.sdpa_backward(on["q"], on["k"], on["v"], on["out"], on["lse"], on["dout"], on["mask"], case["is_causal"], matrix_core=True)
    assert _counts(MFMA, VALU) == (before[0] + 1, before[1])
    return dict(zip(("dq", "dk", "dv"), grads))


@pytest.mark.parametrize("mask", [None, "causal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_matches_the_float64_formulas(ops, golden, shape, mask):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    want = _attention.sdpa_formulas(case)
    if shape[3] == 1:
        # One key: p = 1 and dout . v = delta, so dq and dk are identically zero in exact arithmetic; the float64 formulas leave their
        # own rounding there (1e-17), and the exact value stands in so that _attention.zero_reference_bound applies as it documents.
        assert max(float(want[name].abs().max()) for name in ("dq", "dk")) < 1e-12
        want = dict(want, dq=torch.zeros_like(want["dq"]), dk=torch.zeros_like(want["dk"]))
    _attention.assert_sdpa_matches(f"bwd mfma {shape} {mask}", _backward(ops, case), want, case, ("dq", "dk", "dv"))


@pytest.mark.parametrize("form", ["LL", "N1LL", "NHLL", "transposed"])
@pytest.mark.parametrize("kind", ["bool", "float"])
def test_masks_and_exact_zeros(ops, golden, kind, form, shape=(2, 2, 33, 47, 8)):
    """Fully masked query rows and key columns at both ends and across a wave's edge: exactly 0 in ``dq`` and in ``dk`` / ``dv``."""
    N, H, Lq, Lk, _ = shape
    rows, columns, off = [0, 15, 16, Lq - 1], [0, 15, 16, Lk - 1], False if kind == "bool" else -math.inf
    forms = {"LL": (Lq, Lk), "N1LL": (N, 1, Lq, Lk), "NHLL": (N, H, Lq, Lk), "transposed": (N, H, Lk, Lq)}
    case = _attention.kernel_case(golden("attention"), shape, kind, forms[form])
    if form == "transposed":
        case["mask"] = case["mask"].transpose(-1, -2)
    case["mask"][..., rows, :] = off
    case["mask"][..., columns] = off
    got = _backward(ops, case)
    assert not got["dq"][:, rows].any() and not got["dk"][:, columns].any() and not got["dv"][:, columns].any() and got["dq"].any()
    _attention.assert_sdpa_matches(f"bwd mfma {kind} {form}", got, _attention.sdpa_formulas(case), case, ("dq", "dk", "dv"))


@pytest.mark.parametrize("forward_too", [True, False])
@pytest.mark.parametrize("shape,mask", [((2, 2, 33, 33, 24), "causal"), ((1, 2, 65, 130, 32), "bool")])
def test_autograd_reaches_the_new_backward(ops, golden, shape, mask, forward_too):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    q, k, v = (case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v"))
    before = _counts("cusrl_sdpa_fwd_mfma", MFMA, VALU)
    out = ops.sdpa(q, k, v, attn_mask=None if case["mask"] is None else case["mask"].to(DEV), is_causal=case["is_causal"],
                   matrix_core=forward_too, matrix_core_backward=True)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case["dout"].to(DEV))
    assert _counts("cusrl_sdpa_fwd_mfma", MFMA, VALU) == (before[0] + forward_too, before[1] + 1, before[2])
    _attention.assert_sdpa_matches(f"bwd mfma grad {shape}", {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}, _attention.sdpa_formulas(case), case)


def test_a_module_reaches_both_kernels_through_the_context(ops):
    import cusrl_amd as cusrl

    torch.manual_seed(11)
    module = cusrl.MultiheadSelfAttention(embed_dim=32, num_heads=2).to(DEV)
    x = torch.randn(2, 40, 32, device=DEV)

    def run():
        leaf = x.clone().requires_grad_(True)
        out = module(leaf, is_causal=True)
        return [out.detach(), *torch.autograd.grad(out.sum(), [leaf, *module.parameters()])]

    before = _counts("cusrl_sdpa_fwd_mfma", MFMA, VALU)
    outside = run()
    with ops.matrix_core_attention(backward=True):
        inside = run()
    assert _counts("cusrl_sdpa_fwd_mfma", MFMA, VALU) == (before[0] + 1, before[1] + 1, before[2] + 1)
    errors = [_attention.relative_to_largest(a, b) for a, b in zip(inside, outside)]
    print(f"module inside the context against outside it: worst {max(errors):.3e} of the largest entry")
    assert max(errors) <= _attention.BOUND, errors


def test_a_rows_bits_are_its_own_and_views_give_the_bits_of_their_copies(ops, golden):
    case = _attention.kernel_case(golden("attention"), (2, 3, 65, 47, 20), "float")
    full, again, on = _backward(ops, case), _backward(ops, case), _device(case, ops)
    assert all(torch.equal(full[name], again[name]) for name in full)
    alone = {name: on[name][1:2, :, 2:3].contiguous() for name in ("q", "k", "v", "dout", "out")}
    one = _backward(ops, case, **alone, lse=on["lse"][1:2, 2:3].contiguous(), mask=on["mask"][1:2, 2:3].contiguous())
    assert all(torch.equal(one[name][0, :, 0], full[name][1, :, 2]) for name in full)
    case = _attention.kernel_case(golden("attention"), (2, 3, 19, 19, 8), "causal")
    plain, on = _backward(ops, case), _device(case, ops)
    packed = dict(zip(("q", "k", "v"), torch.stack([on["q"], on["k"], on["v"]], dim=2).unbind(dim=2)))  # the slices of [N, L, 3, H, D]
    first = {name: on[name].transpose(0, 1).contiguous().transpose(0, 1) for name in ("q", "k", "v", "dout")}  # batch_first=False
    for views in (packed, first):
        assert not views["q"].is_contiguous()
        got = _backward(ops, case, **views)
        assert all(torch.equal(got[name], plain[name]) for name in plain)


def _raw(ops, case, shift=None, keep_and_bias=False):
    """The raw entry on 12345-filled outputs and workspace with 64 guard floats on both sides, operand ``shift`` moved by one float."""
    on = _device(case, ops)
    if shift:
        on[shift] = torch.zeros(on[shift].numel() + 4, device=DEV)[1:1 + on[shift].numel()].view(on[shift].shape).copy_(on[shift])
    (N, Lq, H, D), Lk = on["q"].shape, on["k"].shape[1]
    buffers = [torch.full((128 + numel,), 12345.0, device=DEV) for numel in (on["q"].numel(), on["k"].numel(), on["k"].numel(), N * H * Lq)]
    mask = torch.ones(Lq, Lk, device=DEV).data_ptr() if keep_and_bias else None  # (handed in as keep-mask AND bias: refused unread)
    rows = ops.attention._rows_arguments
    status = _native.lib().cusrl_sdpa_bwd_mfma(*rows(on["q"], on["k"], on["v"]), on["out"].data_ptr(), on["lse"].data_ptr(), *rows(on["dout"]),
                                               mask, mask, 0, 0, 0, 0, int(case["is_causal"]), 1.0 / math.sqrt(D),
                                               *(b[64:].data_ptr() for b in buffers), N, H, Lq, Lk, D, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, buffers, on


def test_calls_stay_inside_their_outputs_and_refusals_write_nothing_and_fall_through(ops, golden):
    g = golden("attention")
    for shape, mask in (((2, 3, 33, 47, 8), "causal"), ((1, 2, 17, 16, 128), None)):
        case = _attention.kernel_case(g, shape, mask)
        (status, buffers, _), want = _raw(ops, case), _backward(ops, case)
        assert status == 0 and (buffers[3][64:-64] != 12345.0).all(), "delta fills the workspace"
        for buffer, tensor in zip(buffers, (want["dq"], want["dk"], want["dv"], buffers[3][64:-64])):
            assert (buffer[:64] == 12345.0).all() and (buffer[-64:] == 12345.0).all() and torch.equal(buffer[64:-64], tensor.flatten())
    odd, fine = _attention.kernel_case(g, (2, 3, 5, 7, 6)), _attention.kernel_case(g, (2, 3, 5, 7, 8))
    for case, kwargs, code in ((odd, {}, "E_UNSUPPORTED"), (fine, {"shift": "q"}, "E_UNSUPPORTED"), (fine, {"shift": "dout"}, "E_UNSUPPORTED"),
                               (fine, {"keep_and_bias": True}, "E_INVALID")):
        status, buffers, on = _raw(ops, case, **kwargs)
        assert status == _native._CONSTANTS[code] and all((b == 12345.0).all() for b in buffers), kwargs
        if code == "E_UNSUPPORTED":  # through ops the same operands go on with cusrl_sdpa_bwd
            call = lambda **kw: ops.sdpa_backward(on["q"], on["k"], on["v"], on["out"], on["lse"], on["dout"], **kw)  # noqa: E731
            before = _counts(MFMA, VALU)
            assert all(torch.equal(a, b) for a, b in zip(call(matrix_core=True), call())) and _counts(MFMA, VALU) == (before[0], before[1] + 2)
    assert not ops.sdpa_bwd_mfma_supported(*(odd[n].to(DEV) for n in "qkv")) and ops.sdpa_bwd_mfma_supported(*(fine[n].to(DEV) for n in "qkv"))
