"""Regenerate ``bijectors.npz``: the reference's std bijectors (cusrl/nn/layer/bijector.py:19-146) on CPU in fp32.

    python tests/golden/make_bijectors_golden.py

Recorded for each of the specs ``sigmoid``, ``sigmoid_0.05_1.0``, ``sigmoid_-1_2_0.1``, ``softplus_1_0.01_1``,
``softplus_2_0.05_0.8`` and ``softplus_1_0.01_50`` (the one whose range reaches torch's softplus threshold of 20), under
``<spec>/``:

  * ``class`` and ``repr``       the class name and ``repr()`` of ``make_bijector(spec)`` (its ``extra_repr`` text);
  * ``attr/<name>``              the constructor's attributes (float64);
  * ``forward``                  ``forward(x)``;
  * ``grad``                     the gradient of ``(forward(x) * dy).sum()`` with respect to ``x``;
  * ``inverse``                  ``inverse(y)``;
  * ``float_forward`` / ``float_inverse``   the Python-float forms at ``float_x`` / ``float_y`` (float64).

The shared inputs: ``x`` (a jittered grid over [-30, 60] plus exactly ``float32(min_input)`` and ``float32(max_input)`` of every
softplus spec, no other entry within 4 fp32 ulp of a bound, so that rounding cannot flip the gradient mask: asserted here and
again by the host test), ``dy`` (normal draws), ``y`` (the inverse's inputs, below, inside and above every range).
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
SPECS = ("sigmoid", "sigmoid_0.05_1.0", "sigmoid_-1_2_0.1", "softplus_1_0.01_1", "softplus_2_0.05_0.8", "softplus_1_0.01_50")
ATTRIBUTES = {"SigmoidBijector": ("min_value", "max_value", "range", "eps"),
              "SoftplusBijector": ("scale", "min_value", "max_value", "min_input", "max_input")}
FLOAT_X = (-30.0, -5.0, -1.0, -0.25, 0.0, 0.3, 1.0, 4.0, 25.0, 60.0)
FLOAT_Y = (-1.5, 0.005, 0.05, 0.3, 0.5, 0.99, 1.0, 2.5, 55.0)
MASK_MARGIN_ULP = 4


def bounds_of(bijectors) -> np.ndarray:
    """``float32(min_input)`` and ``float32(max_input)`` of every softplus spec."""
    return np.array([getattr(b, name) for b in bijectors.values() if type(b).__name__ == "SoftplusBijector"
                     for name in ("min_input", "max_input")], dtype=np.float32)


def assert_mask_margin(x: np.ndarray, bounds: np.ndarray):
    """Every bound is an entry of ``x``; no other entry lies within ``MASK_MARGIN_ULP`` fp32 ulp of a bound."""
    assert x.dtype == np.float32 and bounds.dtype == np.float32
    for bound in bounds:
        assert (x == bound).any(), f"{bound!r} is not an entry of x"
        others = x[x != bound].astype(np.float64)
        margin = MASK_MARGIN_ULP * float(np.spacing(np.abs(bound)))
        assert (np.abs(others - float(bound)) > margin).all(), f"an entry of x lies within {MASK_MARGIN_ULP} ulp of {bound!r}"


def make_inputs(out, bijectors):
    gen = torch.Generator().manual_seed(9100)
    grid = torch.linspace(-30.0, 60.0, 181)
    jitter = (torch.rand(181, generator=gen) - 0.5) * 0.4
    jitter[0] = jitter[-1] = 0.0  # (the ends of the span stay where they are)
    bounds = bounds_of(bijectors)
    x = np.unique(np.concatenate([np_(grid + jitter).astype(np.float32), bounds]))
    x = x[torch.randperm(x.size, generator=gen).numpy()]  # (no order a kernel could lean on)
    assert_mask_margin(x, bounds)
    assert x.min() == -30.0 and x.max() == 60.0 and 180 <= x.size <= 200
    out["x"] = x
    out["dy"] = np_(torch.randn(x.size, generator=gen))
    out["y"] = np.concatenate([np.linspace(-2.0, 3.0, 101), [5.0, 20.0, 50.0, 60.0]]).astype(np.float32)
    out["float_x"], out["float_y"] = np.array(FLOAT_X, np.float64), np.array(FLOAT_Y, np.float64)


def record(out, spec, bijector):
    prefix = spec + "/"
    name = type(bijector).__name__
    out[prefix + "class"], out[prefix + "repr"] = np.array(name), np.array(repr(bijector))
    for attribute in ATTRIBUTES[name]:
        out[prefix + "attr/" + attribute] = np.float64(getattr(bijector, attribute))
    x = torch.from_numpy(out["x"].copy()).requires_grad_(True)
    forward = bijector(x)
    (grad,) = torch.autograd.grad((forward * torch.from_numpy(out["dy"].copy())).sum(), x)
    out[prefix + "forward"], out[prefix + "grad"] = np_(forward), np_(grad)
    out[prefix + "inverse"] = np_(bijector.inverse(torch.from_numpy(out["y"].copy())))
    out[prefix + "float_forward"] = np.array([bijector(value) for value in FLOAT_X], np.float64)
    out[prefix + "float_inverse"] = np.array([bijector.inverse(value) for value in FLOAT_Y], np.float64)
    assert all(a.dtype == np.float32 for a in (out[prefix + "forward"], out[prefix + "grad"], out[prefix + "inverse"]))


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    from cusrl.nn.layer.bijector import make_bijector  # noqa: PLC0415

    bijectors = {spec: make_bijector(spec) for spec in SPECS}
    out = dict(META)
    out["specs"] = np.array(SPECS, dtype=np.str_)
    make_inputs(out, bijectors)
    for spec, bijector in bijectors.items():
        record(out, spec, bijector)
    np.savez_compressed(HERE / "bijectors.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("bijectors.npz:", len(out), "arrays,", (HERE / "bijectors.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
