"""``cusrl_band_sdpa_bwd_mfma`` on an MI355X against the float64 band formulas of include/cusrl_hip.h (``_causal_attention.band_formulas``),
bound ``BOUND`` of the float64 tensor's largest entry, on ``out`` / ``lse`` of ``cusrl_band_sdpa_fwd``: the 16-row tile's, the 16-row
sub-tile's and the d-block's edges in both passes, the stride loop, every side tensor, ``key_grad_from`` on and off a tile edge, dead
rows and unseen keys, autograd, row independence, views, guards, refusals and one module.  Every comparison prints what it measured.
Worst measured on an MI355X over all of it, relative to the largest entry: ``dq`` 8.5e-7, ``dk`` 9.9e-7, ``dv`` 1.01e-6; the module's
output and gradients inside the context against outside it: 3.8e-7."""

import math

import pytest
import torch

import _causal_attention as _ca
from cusrl_amd import _native

pytestmark = pytest.mark.gpu
DEV, SYMBOLS = "cuda:0", ("cusrl_band_sdpa_bwd_mfma", "cusrl_band_sdpa_bwd", "cusrl_band_sdpa_fwd_mfma", "cusrl_band_sdpa_fwd")
MID = (2, 2, 33, 17, 20)  # (N, H, Lq, W, D): every axis's edges against this setting; the last shape's 4176 items exceed 4 * 4 * 256
SHAPES = list(dict.fromkeys([MID[:2] + (Lq,) + MID[3:] for Lq in (2, 15, 16, 17, 33)] + [MID[:3] + (W, MID[4]) for W in (1, 15, 16, 17, 33)]
                            + [MID[:4] + (D,) for D in (4, 12, 16, 20, 64, 128)] + [(1, 1, 2, 1, 4), (261, 8, 17, 3, 4)]))
CASES = ([(shape, option, start) for shape in SHAPES for option in ("plain", "all") for start in (0, shape[3])]
         + [(MID, option, start) for option in ("valid", "segments", "slopes") for start in (0, MID[3])]
         + [(MID, option, start) for option in ("plain", "all") for start in (5, 16)])


@pytest.fixture(scope="module")
def ops():
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd.ops


def _counts():
    return tuple(_native.launch_counts.get(symbol, 0) for symbol in SYMBOLS)


def _device(ops, case) -> dict:  # the case's operands on the device with ``out`` / ``lse`` of one ``cusrl_band_sdpa_fwd`` launch
    on = {name: case[name].to(DEV) for name in ("q", "k", "v", "dout")}
    on["sides"] = tuple(None if case[name] is None else case[name].to(DEV) for name in ("key_valid", "q_segment", "alibi_slopes"))
    on["out"], on["lse"] = ops.band_attention._launch_band_fwd(on["q"], on["k"], on["v"], case["window"], *on["sides"], False)
    return on


def _backward(ops, case, taken=True, **views) -> dict:
    """``dq``, ``dk``, ``dv`` of one ``ops.band_sdpa_backward(matrix_core=True)`` call (``views``: device tensors in the operands' place)."""
    on = {**_device(ops, case), **views}
    before = _counts()
    grads = ops.band_sdpa_backward(on["q"], on["k"], on["v"], on["out"], on["lse"], on["dout"], case["window"], *on["sides"],
                                   key_grad_from=case["key_grad_from"], matrix_core=True)
    assert _counts() == (before[0] + taken, before[1] + (not taken), *before[2:])
    return dict(zip(("dq", "dk", "dv"), grads))


@pytest.mark.parametrize("shape,option,start", CASES, ids=lambda s: str(s) if not isinstance(s, tuple) else "x".join(map(str, s)))
def test_backward_matches_the_float64_formulas(ops, golden, shape, option, start):
    case = _ca.kernel_case(golden("attention"), shape, option, start)
    _ca.assert_sdpa_matches(f"band bwd mfma {shape} {option} from {start}", _backward(ops, case), _ca.band_formulas(case), case, ("dq", "dk", "dv"))


@pytest.mark.parametrize("shape", [(2, 2, 33, 5, 8), (1, 2, 40, 17, 20)], ids=lambda s: "x".join(map(str, s)))
def test_dead_rows_and_unseen_keys_get_exact_zeros(ops, golden, shape):
    """Query rows 0, 15, 16 and the last lose every key of their windows through ``key_valid``, and no query sees those keys."""
    Lq, W = shape[2:4]
    case = _ca.kernel_case(golden("attention"), shape, "slopes")
    case["key_valid"] = torch.ones(shape[0], Lq + W, dtype=torch.bool)
    for row in (rows := [0, 15, 16, Lq - 1]):
        case["key_valid"][:, row:row + W + 1] = False
    got, unseen = _backward(ops, case), ~case["key_valid"][0].to(DEV)
    assert not got["dq"][:, rows].any() and not got["dk"][:, unseen].any() and not got["dv"][:, unseen].any() and got["dq"].any()
    _ca.assert_sdpa_matches(f"band bwd mfma dead rows {shape}", got, _ca.band_formulas(case), case, ("dq", "dk", "dv"))


@pytest.mark.parametrize("shape,start", [((2, 2, 33, 17, 24), 0), ((1, 2, 40, 16, 32), 16)])
def test_autograd_reaches_both_matrix_core_kernels(ops, golden, shape, start):
    case = _ca.kernel_case(golden("attention"), shape, "all", start)
    q, k, v = (case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v"))
    sides, before = _device(ops, case)["sides"], _counts()
    out = ops.band_sdpa(q, k, v, case["window"], *sides, key_grad_from=start, matrix_core=True, matrix_core_backward=True)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case["dout"].to(DEV))
    assert _counts() == (before[0] + 1, before[1], before[2] + 1, before[3]) and not dk[:, :start].any() and not dv[:, :start].any()
    got = {"out": out.detach(), "dq": dq, "dk": dk[:, start:], "dv": dv[:, start:]}
    _ca.assert_sdpa_matches(f"band bwd mfma grad {shape} from {start}", got, _ca.band_formulas(case), case)


def test_a_rows_bits_are_its_own_and_views_give_the_bits_of_their_copies(ops, golden):
    case = _ca.kernel_case(golden("attention"), (2, 3, 37, 19, 20), "all", 5)
    full, again, on = _backward(ops, case), _backward(ops, case), _device(ops, case)
    assert all(torch.equal(full[name], again[name]) for name in full)
    alone = {name: on[name][1:2, :, 2:3].contiguous() for name in ("q", "k", "v", "dout", "out")}
    one = _backward(ops, case, **alone, lse=on["lse"][1:2, 2:3].contiguous(), sides=(on["sides"][0][1:2], on["sides"][1][1:2], on["sides"][2][2:3]))
    assert all(torch.equal(one[name][0, :, 0], full[name][1, :, 2]) for name in full)
    k, v = torch.stack([on["k"], on["v"]], dim=2).unbind(dim=2)  # the slices of a packed [N, Lk, 2, H, D] projection
    q = on["q"].transpose(0, 1).contiguous().transpose(0, 1)  # the [L, N, H, D] memory of a sequence-first module
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    views = _backward(ops, case, q=q, k=k, v=v)
    assert all(torch.equal(views[name], full[name]) for name in full)


def _raw(ops, case, shift=False):
    """The raw entry on 12345-filled outputs and workspace with 64 guard floats on both sides, ``q`` moved by one float (``shift``)."""
    on = _device(ops, case)
    if shift:
        on["q"] = torch.zeros(on["q"].numel() + 4, device=DEV)[1:1 + on["q"].numel()].view(on["q"].shape).copy_(on["q"])
    (N, Lq, H, D), W, start = on["q"].shape, case["window"], case["key_grad_from"]
    rows_out = N * (Lq + W - start) * H * D
    buffers = [torch.full((128 + numel,), 12345.0, device=DEV) for numel in (on["q"].numel(), rows_out, rows_out, N * H * Lq)]
    rows = ops.attention._rows_arguments
    status = _native.lib().cusrl_band_sdpa_bwd_mfma(*rows(on["q"], on["k"], on["v"]), *(None if side is None else side.data_ptr() for side in on["sides"]),
                                                    1.0 / math.sqrt(D), on["out"].data_ptr(), on["lse"].data_ptr(), *rows(on["dout"]), start,
                                                    *(b[64:].data_ptr() for b in buffers), N, H, Lq, W, D, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, buffers, on


def test_calls_stay_inside_their_outputs_and_refusals_write_nothing_and_fall_through(ops, golden):
    g = golden("attention")
    for shape, start in (((2, 3, 33, 17, 8), 5), ((1, 2, 17, 16, 128), 16)):
        case = _ca.kernel_case(g, shape, "all", start)
        (status, buffers, _), want = _raw(ops, case), _backward(ops, case)
        assert status == 0 and (buffers[3][64:-64] != 12345.0).all(), "delta fills the workspace"
        for buffer, tensor in zip(buffers, (want["dq"], want["dk"], want["dv"], buffers[3][64:-64])):
            assert (buffer[:64] == 12345.0).all() and (buffer[-64:] == 12345.0).all() and torch.equal(buffer[64:-64], tensor.flatten())
    odd, fine, step = (_ca.kernel_case(g, shape, "all", 3) for shape in ((2, 3, 5, 7, 6), (2, 3, 5, 7, 8), (2, 3, 1, 7, 8)))
    for case, shift in ((odd, False), (fine, True), (step, False)):
        status, buffers, on = _raw(ops, case, shift)
        assert status == _native._CONSTANTS["E_UNSUPPORTED"] and all((b == 12345.0).all() for b in buffers), (case["q"].shape, shift)
        assert not ops.band_sdpa_bwd_mfma_supported(on["q"], on["k"], on["v"], 7, *on["sides"])
        plain = ops.band_sdpa_backward(on["q"], on["k"], on["v"], on["out"], on["lse"], on["dout"], 7, *on["sides"], key_grad_from=3)
        assert all(torch.equal(a, b) for a, b in zip(_backward(ops, case, taken=False, q=on["q"]).values(), plain))  # cusrl_band_sdpa_bwd
    assert ops.band_sdpa_bwd_mfma_supported(*(fine[n].to(DEV) for n in "qkv"), 7)


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
    assert _counts() == (before[0], before[1] + 1, before[2], before[3] + 1), "nothing is routed to the MFMA kernels by default"
    with ops.matrix_core_attention(backward=True):
        inside = run()
    assert _counts() == (before[0] + 1, before[1] + 1, before[2] + 1, before[3] + 1)
    errors = [_ca.relative_to_largest(a, b) for a, b in zip(inside, outside)]
    print(f"causal module inside the context against outside it: worst {max(errors):.3e} of the largest entry")
    assert max(errors) <= _ca.BOUND, errors
