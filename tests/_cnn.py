"""What the Cnn / SeparableConv2d / 2-D encoding tests of both kinds share: the recorded modules (golden ``cnn.npz``), the operands
of the kernel cases, the depthwise-convolution formulas of include/cusrl_hip.h evaluated in any dtype on the CPU (float64: the
expectation; float32: a restatement that shows without a GPU that the bounds are reachable) and the assertions."""

from __future__ import annotations

import numpy as np
import torch
from torch import nn

from _gates import recorded_state, relative_to_largest, run_module  # noqa: F401  (shared with the gate tests)

BOUND = 1e-5  # the standing bound, relative to the largest entry
SYMBOLS = ("cusrl_dwconv2d_fwd", "cusrl_dwconv2d_bwd_input", "cusrl_dwconv2d_bwd_params", "cusrl_dwconv2d_num_partials")
LAUNCHES = SYMBOLS[:3]
# label -> (H, W, (KH, KW, SH, SW, PH, PW, DH, DW), with bias)
GEOMETRIES = {
    "1x1 k1": (1, 1, (1, 1, 1, 1, 0, 0, 1, 1), True),
    "5x7 k3": (5, 7, (3, 3, 1, 1, 0, 0, 1, 1), True),
    "17x16 k7 p3": (17, 16, (7, 7, 1, 1, 3, 3, 1, 1), True),  # the 49-tap limit
    # stride remainders, a padding wider than half the kernel, whole windows inside the padding
    "33x9 k(5,3) s(2,1) p(2,3) d(2,1)": (33, 9, (5, 3, 2, 1, 2, 3, 2, 1), True),
    "8x8 k3 s2": (8, 8, (3, 3, 2, 2, 0, 0, 1, 1), True),  # the last row and column are read by no window
    "5x5 k5": (5, 5, (5, 5, 1, 1, 0, 0, 1, 1), True),  # Ho = Wo = 1
    "6x4 k3 p1 no bias": (6, 4, (3, 3, 1, 1, 1, 1, 1, 1), False),  # W = 4
    "6x5 k(3,2) p1": (6, 5, (3, 2, 1, 1, 1, 1, 1, 1), True),  # W = 5
}
BATCHES = ((1, 1), (3, 3), (130, 3), (2, 8))  # (N, C)
KERNEL_CASES = [(label, N, C) for label in GEOMETRIES for N, C in BATCHES]
STEPS = {"x": 1, "w": 3, "bias": 5, "dout": 7}  # (operand i of a case is pool[(step i + offset) % P]: P is prime)
OFFSETS = {"x": 0, "w": 1201, "bias": 2503, "dout": 3571}

# the recorded modules: tests/golden/make_cnn_golden.py builds the same ones from the reference's classes
SEPARABLE = {
    "k3": (3, 5, 3, {}),
    "stride2": (4, 4, 3, {"stride": 2, "padding": 1}),
    "dilated": (2, 3, (5, 3), {"padding": (2, 1), "dilation": (1, 2)}),
    "nobias": (3, 2, 3, {"bias": False}),
    "same": (3, 4, 3, {"padding": "same"}),
    "reflect": (3, 4, 3, {"padding": 1, "padding_mode": "reflect"}),
}
CNNS = {
    "flat": (lambda Sep: [Sep(1, 4, 3, padding=1), nn.ReLU(), Sep(4, 4, 3, stride=2)], {"input_shape": (6, 6), "output_dim": 16}),
    "image": (lambda Sep: [Sep(2, 4, 3, padding=1), nn.ReLU(), Sep(4, 3, 3)],
              {"input_shape": (2, 6, 6), "input_flattened": False, "flatten_output": False}),
    "mixed": (lambda Sep: [nn.Conv2d(1, 3, 3, padding=1), nn.MaxPool2d(2), Sep(3, 4, 3, padding=1), nn.ReLU(), Sep(4, 2, 2)],
              {"input_shape": (8, 8)}),
}
MODULE_CASES = [*(("sep", name) for name in SEPARABLE), *(("cnn", name) for name in CNNS)]
DEVICE_MODULE_CASES = [case for case in MODULE_CASES if case not in (("sep", "reflect"), ("cnn", "mixed"))]
SINUSOIDAL = {"8x5x7": ((8, 5, 7), {}), "4x1x3": ((4, 1, 3), {"base": 100})}
LEARNABLE = (4, 5, 7)


# ------------------------------------------------------------------------------------------------ kernel operands
def cut(g, name: str, shape) -> torch.Tensor:
    """fp32 operand ``name``: element i (row-major) is ``pool[(step i + offset) % P]``."""
    pool = g["kernel_pool"]
    index = (np.arange(int(np.prod(shape)), dtype=np.int64) * STEPS[name] + OFFSETS[name]) % pool.size
    return torch.from_numpy(np.ascontiguousarray(pool[index])).view(*shape)


def output_size(H: int, W: int, geometry) -> tuple[int, int]:
    KH, KW, SH, SW, PH, PW, DH, DW = geometry
    return (H + 2 * PH - DH * (KH - 1) - 1) // SH + 1, (W + 2 * PW - DW * (KW - 1) - 1) // SW + 1


def kernel_case(g, label: str, N: int, C: int) -> dict:
    """``x [N, C, H, W]``, ``w [C, 1, KH, KW]``, ``bias [C]`` or None, ``dout [N, C, Ho, Wo]`` and the ``geometry``."""
    H, W, geometry, with_bias = GEOMETRIES[label]
    Ho, Wo = output_size(H, W, geometry)
    return {"x": cut(g, "x", (N, C, H, W)), "w": cut(g, "w", (C, 1, geometry[0], geometry[1])),
            "bias": cut(g, "bias", (C,)) if with_bias else None, "dout": cut(g, "dout", (N, C, Ho, Wo)), "geometry": geometry}


# ------------------------------------------------------------------------------------------------ the formulas, in any dtype
def _windows(padded, ky, kx, Ho, Wo, geometry):
    """What tap (ky, kx) reads of the zero-padded image, one entry per output position: a strided view."""
    _, _, SH, SW, _, _, DH, DW = geometry
    return padded[:, :, ky * DH: ky * DH + (Ho - 1) * SH + 1: SH, kx * DW: kx * DW + (Wo - 1) * SW + 1: SW]


def dwconv_formulas(case: dict, dtype, magnitudes: bool = False) -> dict:
    """``out``, ``dx``, ``dw`` and ``dbias`` (None without a bias) by the formulas of include/cusrl_hip.h, every step in ``dtype``
    and the terms of ``out`` / ``dx`` added in the kernel's order (the bias, then the taps by (ky, kx)).  ``magnitudes``: the
    same sums over the absolute values of the terms — what the error bound of ``out`` and ``dx`` is a multiple of."""
    prepare = (lambda t: t.cpu().to(dtype).abs()) if magnitudes else (lambda t: t.cpu().to(dtype))
    x, w, dout = prepare(case["x"]), prepare(case["w"]), prepare(case["dout"])
    bias = None if case["bias"] is None else prepare(case["bias"])
    KH, KW, SH, SW, PH, PW, DH, DW = case["geometry"]
    N, C, H, W = x.shape
    Ho, Wo = dout.shape[2:]
    padded = torch.zeros(N, C, H + 2 * PH, W + 2 * PW, dtype=dtype)
    padded[:, :, PH:PH + H, PW:PW + W] = x
    dx_padded = torch.zeros_like(padded)
    out = torch.zeros(N, C, Ho, Wo, dtype=dtype) if bias is None else bias.view(1, C, 1, 1).expand(N, C, Ho, Wo).clone()
    dw = torch.zeros(C, 1, KH, KW, dtype=dtype)
    for ky in range(KH):
        for kx in range(KW):
            tap = w[:, 0, ky, kx].view(1, C, 1, 1)
            window = _windows(padded, ky, kx, Ho, Wo, case["geometry"])
            out = out + tap * window
            target = _windows(dx_padded, ky, kx, Ho, Wo, case["geometry"])
            target.copy_(target + tap * dout)  # (the windows of one tap do not overlap: strides are at least 1)
            dw[:, 0, ky, kx] = (dout * window).sum(dim=(0, 2, 3))
    return {"out": out, "dx": dx_padded[:, :, PH:PH + H, PW:PW + W].contiguous(), "dw": dw,
            "dbias": None if bias is None else dout.sum(dim=(0, 2, 3))}


def unread_positions(case: dict) -> torch.Tensor:
    """bool ``[H, W]``: the input positions no window reads (their gradient is the empty sum)."""
    ones = {"x": torch.ones_like(case["x"][:1, :1]), "w": torch.ones_like(case["w"][:1]), "bias": None,
            "dout": torch.ones_like(case["dout"][:1, :1]), "geometry": case["geometry"]}
    return dwconv_formulas(ones, torch.float64)["dx"][0, 0] == 0


def gamma(n: int) -> float:
    """Higham's constant for a sum of n fp32 terms: n u / (1 - n u), u = 2^-24."""
    u = 2.0 ** -24
    return n * u / (1 - n * u)


# ------------------------------------------------------------------------------------------------ assertions
def assert_kernel_matches(label: str, got: dict, case: dict) -> dict:
    """``out`` and ``dx``: per element ``|got - float64| <= gamma(K + 1) * sum |terms|`` with K the tap count (holds for fp32
    summation in any order, with or without fma).  ``dw`` and ``dbias``: within 1e-5 of the tensor's largest entry.  Prints and
    returns what was measured: ``out`` / ``dx`` as the largest fraction of the bound, ``dw`` / ``dbias`` relative to the largest
    entry."""
    want = dwconv_formulas(case, torch.float64)
    terms = dwconv_formulas(case, torch.float64, magnitudes=True)
    factor = gamma(case["geometry"][0] * case["geometry"][1] + 1)
    errors = {}
    for name in ("out", "dx", "dw", "dbias"):
        if want[name] is None:
            assert got.get(name) is None, f"{label} {name}: no bias, no gradient of one"
            continue
        candidate = got[name].detach().cpu()
        assert candidate.dtype == torch.float32 and candidate.shape == want[name].shape, f"{label} {name}: {candidate.shape}"
        assert torch.isfinite(candidate).all(), f"{label} {name}: not finite"
        if name in ("out", "dx"):
            error, bound = (candidate.double() - want[name]).abs(), factor * terms[name]
            assert torch.equal(candidate[bound == 0], torch.zeros_like(candidate[bound == 0])), f"{label} {name}: an empty sum is not 0"
            errors[name] = float((error[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        else:
            errors[name] = relative_to_largest(candidate, want[name].numpy())
    print(f"{label}: " + ", ".join(f"{name} {error:.3e}" for name, error in errors.items()) + "  (out, dx: fraction of the bound)")
    for name, error in errors.items():
        limit = 1.0 if name in ("out", "dx") else BOUND
        assert error <= limit, f"{label} {name}: {error:.3e} exceeds {limit:.0e}"
    return errors


# ------------------------------------------------------------------------------------------------ recorded modules
def build_module(cusrl, family: str, name: str):
    """The recorded module with this project's classes (weights not loaded yet)."""
    if family == "sep":
        cin, cout, kernel, kwargs = SEPARABLE[name]
        return cusrl.nn.SeparableConv2d(cin, cout, kernel, **kwargs)
    layers, kwargs = CNNS[name]
    return cusrl.nn.Cnn(layers(cusrl.nn.SeparableConv2d), **kwargs)


def module_inputs(g, family: str, name: str) -> tuple[dict, torch.Tensor]:
    """(the recorded input by name, the weight ``w`` of the recorded objective ``(out * w).sum()``)."""
    return {"input": torch.from_numpy(g[f"{family}_input/{name}"].copy())}, torch.from_numpy(g[f"{family}_w/{name}"].copy())


def assert_module_matches(label: str, got: dict, g, prefix: str) -> dict:
    """Every recorded tensor within 1e-5 of its largest entry, and exactly zero where the recorded tensor is."""
    recorded = {key[len(prefix):]: g[key] for key in g.files if key.startswith(prefix) and not key[len(prefix):].startswith("state")}
    assert sorted(got) == sorted(recorded), (sorted(got), sorted(recorded))
    errors = {key: relative_to_largest(got[key], value) for key, value in recorded.items()}
    print(f"{label}: worst {max(errors.values()):.3e} of the largest entry over {len(errors)} tensors")
    for key, error in errors.items():
        assert error <= BOUND, f"{label} {key}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
        assert not got[key].detach().cpu().numpy()[recorded[key] == 0].any(), f"{label} {key}: not zero where the record is"
    return errors
