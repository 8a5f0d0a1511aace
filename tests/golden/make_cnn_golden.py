"""Regenerate ``cnn.npz``: the reference's ``SeparableConv2d`` (cusrl/nn/layer/separable_conv.py:7-85), ``Cnn``
(cusrl/nn/module/cnn.py:13-108) and 2-D positional encodings (cusrl/nn/layer/encoding.py:11-106) on CPU, plus the pool the kernel
cases are cut from.

    python tests/golden/make_cnn_golden.py

Recorded, all with seeded weights and as the reference computes them in fp32:

  * ``sep/<case>/``   ``SeparableConv2d`` in the configurations of ``SEPARABLE`` (tests/_cnn.py builds the same ones) on
                 ``[6, C, 9, 11]``: the state dict as constructed, ``out`` and the gradients of ``(out * w).sum()`` with respect to
                 the input and every parameter;
  * ``cnn/<case>/``   ``Cnn`` over ``[SeparableConv2d, ReLU, SeparableConv2d]`` in the variants of ``CNNS``: the same records;
  * ``pe/``           the sinusoidal tables for ``(C, H, W) = (8, 5, 7)`` and ``(4, 1, 3)`` with ``base=100``, the learnable
                 layer's ``pe`` under a recorded seed, and one output of each layer.

The kernel cases are inputs only: one pool of normal draws of prime length (tests/_cnn.py cuts every operand from it by an index
rule); their expectations are float64 evaluations of the formulas, made by the tests.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_gates_golden import record_module  # noqa: E402
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
POOL = 8191  # (prime)
SEP_INPUT = (6, 9, 11)  # N, H, W
# case -> (in_channels, out_channels, kernel_size, keyword arguments)
SEPARABLE = {
    "k3": (3, 5, 3, {}),
    "stride2": (4, 4, 3, {"stride": 2, "padding": 1}),
    "dilated": (2, 3, (5, 3), {"padding": (2, 1), "dilation": (1, 2)}),
    "nobias": (3, 2, 3, {"bias": False}),
    "same": (3, 4, 3, {"padding": "same"}),
    "reflect": (3, 4, 3, {"padding": 1, "padding_mode": "reflect"}),
}
# case -> (layers(SeparableConv2d), keyword arguments of Cnn, input shape)
CNNS = {
    "flat": (lambda Sep: [Sep(1, 4, 3, padding=1), nn.ReLU(), Sep(4, 4, 3, stride=2)], {"input_shape": (6, 6), "output_dim": 16}, (5, 3, 36)),
    "image": (lambda Sep: [Sep(2, 4, 3, padding=1), nn.ReLU(), Sep(4, 3, 3)],
              {"input_shape": (2, 6, 6), "input_flattened": False, "flatten_output": False}, (4, 2, 6, 6)),
    "mixed": (lambda Sep: [nn.Conv2d(1, 3, 3, padding=1), nn.MaxPool2d(2), Sep(3, 4, 3, padding=1), nn.ReLU(), Sep(4, 2, 2)],
              {"input_shape": (8, 8)}, (3, 64)),
}
SINUSOIDAL = {"8x5x7": ((8, 5, 7), {}), "4x1x3": ((4, 1, 3), {"base": 100})}
LEARNABLE = (4, 5, 7)
LEARNABLE_SEED = 9300


def make_separable(out):
    from cusrl.nn.layer.separable_conv import SeparableConv2d  # noqa: PLC0415

    N, H, W = SEP_INPUT
    for index, (name, (cin, cout, kernel, kwargs)) in enumerate(SEPARABLE.items()):
        torch.manual_seed(7100 + index)
        module = SeparableConv2d(cin, cout, kernel, **kwargs)
        gen = torch.Generator().manual_seed(7200 + index)
        x = torch.randn(N, cin, H, W, generator=gen)
        w = torch.randn(module(x).shape, generator=gen)
        out[f"sep_input/{name}"], out[f"sep_w/{name}"] = np_(x), np_(w)
        record_module(out, f"sep/{name}/", module, {"input": x}, w)


def make_cnns(out):
    from cusrl.nn.layer.separable_conv import SeparableConv2d  # noqa: PLC0415
    from cusrl.nn.module.cnn import Cnn  # noqa: PLC0415

    for index, (name, (layers, kwargs, shape)) in enumerate(CNNS.items()):
        torch.manual_seed(8100 + index)
        module = Cnn(layers(SeparableConv2d), **kwargs)
        gen = torch.Generator().manual_seed(8200 + index)
        x = torch.randn(*shape, generator=gen)
        w = torch.randn(module(x).shape, generator=gen)
        out[f"cnn_input/{name}"], out[f"cnn_w/{name}"] = np_(x), np_(w)
        out[f"cnn_dims/{name}"] = np.array([module.input_dim, module.output_dim], dtype=np.int64)
        record_module(out, f"cnn/{name}/", module, {"input": x}, w)


def make_encodings(out):
    from cusrl.nn.layer.encoding import LearnablePositionalEncoding2D, SinusoidalPositionalEncoding2D  # noqa: PLC0415

    gen = torch.Generator().manual_seed(9200)
    for name, ((C, H, W), kwargs) in SINUSOIDAL.items():
        layer = SinusoidalPositionalEncoding2D(C, H, W, **kwargs)
        x = torch.randn(2, 3, C, H, W, generator=gen)
        out[f"pe/sinusoidal/{name}/pe"], out[f"pe/sinusoidal/{name}/x"], out[f"pe/sinusoidal/{name}/out"] = np_(layer.pe), np_(x), np_(layer(x))
        out[f"pe/sinusoidal/{name}/requires_grad"] = np.array(layer.pe.requires_grad)
    torch.manual_seed(LEARNABLE_SEED)
    layer = LearnablePositionalEncoding2D(*LEARNABLE)
    x = torch.randn(2, *LEARNABLE, generator=gen)
    out["pe/learnable/pe"], out["pe/learnable/x"], out["pe/learnable/out"] = np_(layer.pe), np_(x), np_(layer(x))
    out["pe/learnable/requires_grad"] = np.array(layer.pe.requires_grad)
    out["pe/learnable/seed"] = np.array(LEARNABLE_SEED)


def make_kernel_pool(out):
    gen = torch.Generator().manual_seed(779)
    out["kernel_pool"] = np_(torch.randn(POOL, generator=gen))
    assert np.isfinite(out["kernel_pool"]).all() and (np.abs(out["kernel_pool"]) > 1e-30).all()  # no denormal decides a case


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_separable(out)
    make_cnns(out)
    make_encodings(out)
    make_kernel_pool(out)
    np.savez_compressed(HERE / "cnn.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("cnn.npz:", len(out), "arrays,", (HERE / "cnn.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
