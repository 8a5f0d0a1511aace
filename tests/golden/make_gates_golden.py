"""Regenerate ``gates.npz``: the reference's gate layers (cusrl/nn/layer/gate.py:17-154), GLU activations
(cusrl/nn/layer/activation.py:7-26) and ``FeedForward`` (cusrl/nn/layer/transformer.py:12-66) on CPU, plus the pool the kernel
cases are cut from.

    python tests/golden/make_gates_golden.py

Recorded, all with seeded weights and as the reference computes them in fp32:

  * ``gate/<name>/<dim>/``   each of the seven gates (``passthrough``, ``residual``, ``input``, ``output``, ``highway``,
                 ``sigmoid_tanh``, ``gru``) at ``embed_dim`` 8 and 6 (the second is not a multiple of 4): the state dict as
                 constructed (so the biases are the initial fills), ``out`` for ``x``, ``y`` of shape ``[5, 3, dim]`` and the
                 gradients of ``(out * w).sum()`` with respect to ``x``, ``y`` and every parameter (zeros where the output does not
                 depend on an input);
  * ``glu/<name>/<width>/``  ``GeGlu`` and ``SwiGlu`` on ``[7, 12]`` and ``[7, 16]``: output and input gradient;
  * ``ff/<name>/``           ``FeedForward(6, 16, GeGlu)``, ``FeedForward(8, 16, SwiGlu, output_dim=4)`` and the default
                 ``FeedForward(6)`` (GELU) on ``[5, 3, input_dim]``: state dict, output, all gradients.

The kernel cases are inputs only: one pool of normal draws of prime length (tests/_gates.py cuts every operand from it by an
index rule and scales the pre-activations to N(0, 2^2)) and a small saturated set, every combination of p and q in
+-{20, 100}; their expectations are the float64 evaluation of the formulas, made by the tests.
"""

from __future__ import annotations

import itertools
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
T, B = 5, 3
GATES = {"passthrough": None, "residual": "residual", "input": "input", "output": "output", "highway": "highway",
         "sigmoid_tanh": "sigmoid_tanh", "gru": "gru"}
GATE_DIMS = (8, 6)
GLU_SHAPES = ((7, 12), (7, 16))
POOL = 4099  # (prime)
SATURATED = (20.0, -20.0, 100.0, -100.0)


def record_module(out, prefix, module, inputs: dict, weight):
    """State dict, output and the gradients of ``(output * weight).sum()`` with respect to the inputs and every parameter."""
    out[prefix + "state_keys"] = np.array(list(module.state_dict()), dtype=np.str_)
    for key, value in module.state_dict().items():
        out[prefix + "state/" + key] = np_(value)
    leaves = {name: value.clone().requires_grad_(True) for name, value in inputs.items()}
    output = module(*leaves.values())
    params = dict(module.named_parameters())
    wanted = [*leaves.values(), *params.values()]
    grads = torch.autograd.grad((output * weight).sum(), wanted, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(wanted, grads)]
    out[prefix + "out"] = np_(output)
    for name, grad in zip([*("grad_" + n for n in leaves), *("grad/" + n for n in params)], grads):
        out[prefix + name] = np_(grad)


def make_gates(out):
    from cusrl.nn.layer.gate import get_gate_cls  # noqa: PLC0415

    for dim in GATE_DIMS:
        gen = torch.Generator().manual_seed(4100 + dim)
        x, y, w = (torch.randn(T, B, dim, generator=gen) for _ in range(3))
        out[f"gate_x/{dim}"], out[f"gate_y/{dim}"], out[f"gate_w/{dim}"] = np_(x), np_(y), np_(w)
        for index, (name, gate_type) in enumerate(GATES.items()):
            torch.manual_seed(100 * dim + index)
            record_module(out, f"gate/{name}/{dim}/", get_gate_cls(gate_type)(dim), {"x": x, "y": y}, w)


def make_glus(out):
    from cusrl.nn.layer.activation import GeGlu, SwiGlu  # noqa: PLC0415

    for rows, width in GLU_SHAPES:
        gen = torch.Generator().manual_seed(5200 + width)
        input, w = torch.randn(rows, width, generator=gen) * 2, torch.randn(rows, width // 2, generator=gen)
        out[f"glu_input/{width}"], out[f"glu_w/{width}"] = np_(input), np_(w)
        for name, cls in (("geglu", GeGlu), ("swiglu", SwiGlu)):
            record_module(out, f"glu/{name}/{width}/", cls(), {"input": input}, w)


def make_feedforwards(out):
    from cusrl.nn.layer.activation import GeGlu, SwiGlu  # noqa: PLC0415
    from cusrl.nn.layer.transformer import FeedForward  # noqa: PLC0415

    cases = {"geglu": lambda: FeedForward(6, 16, GeGlu), "swiglu": lambda: FeedForward(8, 16, SwiGlu, output_dim=4),
             "gelu": lambda: FeedForward(6)}
    for index, (name, build) in enumerate(cases.items()):
        torch.manual_seed(6300 + index)
        module = build()
        gen = torch.Generator().manual_seed(6400 + index)
        input = torch.randn(T, B, module.input_dim, generator=gen)
        w = torch.randn(T, B, module.output_dim, generator=gen)
        out[f"ff_input/{name}"], out[f"ff_w/{name}"] = np_(input), np_(w)
        record_module(out, f"ff/{name}/", module, {"input": input}, w)


def make_kernel_cases(out):
    gen = torch.Generator().manual_seed(778)
    out["kernel_pool"] = np_(torch.randn(POOL, generator=gen))
    assert np.isfinite(out["kernel_pool"]).all() and (np.abs(out["kernel_pool"]) > 1e-30).all()  # no denormal decides a case
    combos = np.array(list(itertools.product(SATURATED, SATURATED)), dtype=np.float32)  # 16 (p, q) pairs
    out["saturated_p"], out["saturated_q"] = combos[:, 0].copy(), combos[:, 1].copy()


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_gates(out)
    make_glus(out)
    make_feedforwards(out)
    make_kernel_cases(out)
    np.savez_compressed(HERE / "gates.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("gates.npz:", len(out), "arrays,", (HERE / "gates.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
