"""Regenerate ``attention.npz``: the reference's attention layers (cusrl/nn/layer/mha.py:16-391), ``RotaryEmbedding``
(cusrl/nn/layer/encoding.py:128-198) and transformer layers (cusrl/nn/layer/transformer.py:69-402) on CPU, plus the pool the
kernel cases are cut from.

    python tests/golden/make_attention_golden.py

Recorded for every case of ``tests/_attention.py``'s ``MODULE_CASES`` (seeded weights, fp32 as the reference computes them):
``<case>/state_keys`` and ``<case>/state/<key>``, the inputs ``<case>/input/<name>``, the masks ``<case>/call/<argument>``, the
weight ``<case>/w`` and under ``<case>/result/`` the output and the gradients of ``(out * w).sum()`` with respect to every input
and parameter.  The cases: the three attention modules at ``embed_dim`` 8 / 2 heads and 6 / 3 heads (``head_dim`` 2) with no
mask, ``is_causal``, a bool ``(Lq, Lk)`` mask with one fully masked row and a float ``(N, H, Lq, Lk)`` mask, ``batch_first=False``,
every ``qk_norm``, ``rope_base=10000.0``, ``k_dim`` / ``v_dim`` / ``kv_dim`` other than ``embed_dim``, ``Lq != Lk`` for the cross
forms; ``RotaryEmbedding`` with an ``offset`` past its initial cache; ``TransformerEncoderLayer`` at (post, residual, layer),
(pre, gru, rms) and (post, highway, None) with ``input_dim`` / ``output_dim`` projections and ``SwiGlu``;
``TransformerDecoderLayer`` at (post, residual, layer) and (pre, output, layer) with a ``context_dim``.

The kernel cases are inputs only: one pool of normal draws of prime length, from which tests/_attention.py cuts ``q``, ``k``,
``v``, ``dout`` and the masks by an index rule; their expectations are the float64 evaluation of the formulas, made by the tests.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import _attention  # noqa: E402
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
POOL = 4099  # (prime)


def make_modules(out, cusrl):
    for index, (name, (_, _, shapes, call)) in enumerate(_attention.MODULE_CASES.items()):
        torch.manual_seed(9100 + index)
        module = _attention.build_module(cusrl.nn, name)
        gen = torch.Generator().manual_seed(9300 + index)
        inputs = {key: torch.randn(shape, generator=gen) for key, shape in shapes.items()}
        arguments = {key: _attention.make_mask(value, _attention.mask_shape(name, key, value), gen) if isinstance(value, str) else value
                     for key, value in call.items()}
        prefix = name + "/"
        out[prefix + "state_keys"] = np.array(list(module.state_dict()), dtype=np.str_)
        for key, value in module.state_dict().items():
            out[prefix + "state/" + key] = np_(value)
        for key, value in inputs.items():
            out[prefix + "input/" + key] = np_(value)
        for key, value in arguments.items():
            if isinstance(value, torch.Tensor):
                out[prefix + "call/" + key] = np_(value)
        with torch.no_grad():
            shape = module(*inputs.values(), **arguments).shape
        w = torch.randn(shape, generator=gen)
        out[prefix + "w"] = np_(w)
        for key, value in _attention.run_module(module, inputs, arguments, w).items():
            assert torch.isfinite(value).all(), (name, key)
            out[prefix + "result/" + key] = np_(value)


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_modules(out, cusrl)
    gen = torch.Generator().manual_seed(779)
    out["kernel_pool"] = np_(torch.randn(POOL, generator=gen))
    assert np.isfinite(out["kernel_pool"]).all() and (np.abs(out["kernel_pool"]) > 1e-30).all()
    np.savez_compressed(HERE / "attention.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("attention.npz:", len(out), "arrays,", (HERE / "attention.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
