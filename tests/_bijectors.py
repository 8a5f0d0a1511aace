"""What the bijector tests of both kinds share: the recorded runs of the reference (golden ``bijectors.npz``), the reference's torch
expression written out (the fallback's and the comparison's form), the kernel's formulas evaluated in any dtype on the host
(float64: the expectation), the operands of the kernel cases and the error measures."""

from __future__ import annotations

import numpy as np
import torch

BOUND = 1e-5  # the standing bound, relative to the largest entry (tests/test_simba_gpu.py)
SPECS = ("sigmoid", "sigmoid_0.05_1.0", "sigmoid_-1_2_0.1", "softplus_1_0.01_1", "softplus_2_0.05_0.8", "softplus_1_0.01_50")
ROWS = (1, 3, 257, 2049)  # a single row, one block, a ragged last block, several blocks
WIDTHS = (1, 3, 4, 12, 50)  # a single element, the scalar path (n % 4 != 0 where rows is odd), the vector path
ATTRIBUTES = {"SigmoidBijector": ("min_value", "max_value", "range", "eps"),
              "SoftplusBijector": ("scale", "min_value", "max_value", "min_input", "max_input")}
MASK_MARGIN_ULP = 4
SOFTPLUS_THRESHOLD = 20.0  # torch's


def is_softplus(spec: str) -> bool:
    return spec.startswith("softplus")


def attributes(g, spec: str) -> dict[str, float]:
    cls = str(g[spec + "/class"])
    return {name: float(g[f"{spec}/attr/{name}"]) for name in ATTRIBUTES[cls]}


def softplus_bounds(g) -> np.ndarray:
    """``float32(min_input)`` and ``float32(max_input)`` of every softplus spec, as recorded."""
    return np.array([attributes(g, spec)[name] for spec in SPECS if is_softplus(spec) for name in ("min_input", "max_input")],
                    dtype=np.float32)


def assert_mask_margin(x: np.ndarray, bounds: np.ndarray):
    """Every bound is an entry of ``x``; no other entry lies within ``MASK_MARGIN_ULP`` fp32 ulp of a bound (rounding cannot
    flip the gradient mask)."""
    assert x.dtype == np.float32 and bounds.dtype == np.float32
    for bound in bounds:
        assert (x == bound).any(), f"{bound!r} is not an entry of x"
        others = x[x != bound].astype(np.float64)
        margin = MASK_MARGIN_ULP * float(np.spacing(np.abs(bound)))
        assert (np.abs(others - float(bound)) > margin).all(), f"an entry of x lies within {MASK_MARGIN_ULP} ulp of {bound!r}"


# ------------------------------------------------------------------------------------------------ the expressions
def torch_expression(bijector, x: torch.Tensor) -> torch.Tensor:
    """The reference's tensor forward (cusrl/nn/layer/bijector.py:86 and :110-111) from the module's attributes, as torch ops in
    ``x``'s dtype on ``x``'s device."""
    if type(bijector).__name__ == "SigmoidBijector":
        return bijector.min_value + bijector.range * torch.sigmoid(x)
    clamped = x.clamp(bijector.min_input, bijector.max_input)
    return torch.nn.functional.softplus(clamped * bijector.scale) / bijector.scale


class TorchForm(torch.nn.Module):
    """A bijector's stand-in that always evaluates :func:`torch_expression` (never the kernel)."""

    def __init__(self, bijector):
        super().__init__()
        self.inner = bijector

    def forward(self, input):
        return torch_expression(self.inner, input)

    def inverse(self, input):
        return self.inner.inverse(input)


def _f32(value: float) -> float:
    return float(np.float32(value))


def formulas(spec: str, attrs: dict, x: torch.Tensor, dy: torch.Tensor, dtype=torch.float64) -> tuple[torch.Tensor, torch.Tensor]:
    """``(y, dx)`` by include/cusrl_hip.h's formulas, every step in ``dtype`` on the host, with the fp32 roundings of the
    parameters (what the kernel receives and what torch makes of the module's Python floats)."""
    x, dy = x.detach().cpu().to(dtype), dy.detach().cpu().to(dtype)
    if not is_softplus(spec):
        low, span = _f32(attrs["min_value"]), _f32(attrs["range"])
        s = 1 / (1 + torch.exp(-x))
        return low + span * s, dy * span * (1 - s) * s
    scale, low, high = _f32(attrs["scale"]), _f32(attrs["min_input"]), _f32(attrs["max_input"])
    z = x.clamp(low, high) * scale
    y = torch.where(z > SOFTPLUS_THRESHOLD, z, torch.log1p(torch.exp(z))) / scale
    slope = torch.where(z > SOFTPLUS_THRESHOLD, torch.ones_like(z), 1 / (1 + torch.exp(-z)))
    inside = (x >= low) & (x <= high)
    return y, torch.where(inside, dy * slope, torch.zeros_like(dy))


# ------------------------------------------------------------------------------------------------ kernel operands
def edge_values(g) -> np.ndarray:
    """The recorded ``x`` with the softplus bounds in front: [-30, 60], every bound exactly, both sides of torch's threshold."""
    x, bounds = g["x"], softplus_bounds(g)
    return np.concatenate([bounds, x[~np.isin(x, bounds)]]).astype(np.float32)


def kernel_case(g, rows: int, width: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(x, dy)`` of shape ``[rows, width]`` on the CPU: N(0, 3^2) draws with as many :func:`edge_values` as fit written over
    the leading entries, and N(0, 1) draws."""
    gen = torch.Generator().manual_seed(1000 * rows + width)
    n = rows * width
    x = torch.randn(n, generator=gen) * 3.0
    edges = torch.from_numpy(edge_values(g))[:n]
    x[: edges.numel()] = edges
    return x.view(rows, width), torch.randn(n, generator=gen).view(rows, width)


# ------------------------------------------------------------------------------------------------ error measures
def _f64(t) -> np.ndarray:
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def relative_to_largest(candidate, reference) -> float:
    candidate, reference = _f64(candidate), _f64(reference)
    assert candidate.shape == reference.shape, (candidate.shape, reference.shape)
    largest = np.abs(reference).max()
    return float(np.abs(candidate - reference).max() / largest) if largest else float(np.abs(candidate).max())


def ulp_error(candidate, reference) -> float:
    """The largest ``|candidate - reference|`` in units of the fp32 spacing at the (float64) reference value."""
    candidate, reference = _f64(candidate), _f64(reference)
    spacing = np.spacing(np.abs(reference).astype(np.float32)).astype(np.float64)
    return float((np.abs(candidate - reference) / spacing).max())


def differing(candidate, reference) -> int:
    """How many entries are not bit-equal (NaN patterns count as equal where both are NaN)."""
    a = np.ascontiguousarray(candidate.detach().cpu().numpy() if isinstance(candidate, torch.Tensor) else candidate)
    b = np.ascontiguousarray(reference)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.uint32 if a.dtype == np.float32 else np.uint64) != b.view(np.uint32 if b.dtype == np.float32 else np.uint64)).sum())
