"""Regenerate ``causal_attention.npz``: the reference's recurrent transformer modules (``CausalMultiheadSelfAttention`` and
``CausalTransformerEncoderLayer``, cusrl/nn/module/causal_attn.py:49-402) on CPU, through uncompiled flex_attention, and the
values of ``get_alibi_slopes`` / ``compute_segment_ids`` (cusrl/nn/utils/attention.py:16-77).

    python tests/golden/make_causal_attention_golden.py

Recorded for every case of ``tests/_causal_attention.py``'s ``MODULE_CASES`` (seeded weights, fp32 as the reference computes
them): ``<case>/state_keys`` and ``<case>/state/<key>``, under ``<case>/input/`` the input, the warm-up input that produced the
memory (when the case has one) and ``done`` (when it has one), the weight ``<case>/w``, and under ``<case>/result/`` the output,
both memory entries and the gradients of ``(out * w).sum()`` with respect to the input and every parameter.  The cases, each at
``embed_dim`` 8 / 2 heads and 6 / 3 heads (``head_dim`` 2), window 4: no memory; a warm-up shorter than the window (a partly
false cache mask); ``done`` at the first, the last and two consecutive steps; ``L`` below, equal to and above the window; a 2-D
step input; ``sequential=False`` with two batch dimensions; two batch dimensions with ``done``; a sequence-aligned memory with
``done``; ``rope_base=100.0``; ALiBi slopes (``get_alibi_slopes(3)``: not a power of two); both together; ``input_dim`` /
``output_dim`` projections; the layer at (post, residual), (pre, gru), (None, highway) and with ALiBi, RoPE and projections.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import _causal_attention as _ca  # noqa: E402
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    from cusrl.nn.module import causal_attn  # noqa: PLC0415
    from cusrl.nn.utils.attention import compute_segment_ids, get_alibi_slopes  # noqa: PLC0415

    out = dict(META)
    for index, name in enumerate(_ca.MODULE_CASES):
        torch.manual_seed(9500 + index)
        module = _ca.build_module(causal_attn, name, get_alibi_slopes)
        gen = torch.Generator().manual_seed(9700 + index)
        tensors = _ca.make_inputs(name, gen)
        prefix = name + "/"
        out[prefix + "state_keys"] = np.array(list(module.state_dict()), dtype=np.str_)
        for key, value in module.state_dict().items():
            out[prefix + "state/" + key] = np_(value)
        for key, value in tensors.items():
            out[prefix + "input/" + key] = np_(value)
        shape = _ca.run_case(module, name, tensors, None)["out"].shape
        w = torch.randn(shape, generator=gen)
        out[prefix + "w"] = np_(w)
        for key, value in _ca.run_case(module, name, tensors, w).items():
            assert torch.isfinite(value).all(), (name, key)
            if key.startswith("grad") and "norm" not in key:  # (a layer without norms leaves norm1 / norm2 unused)
                assert value.any(), f"{name} {key}: identically zero"
            out[prefix + "result/" + key] = np_(value)
    for heads in (1, 2, 3, 4, 6, 8, 12):
        out[f"alibi_slopes/{heads}"] = np.array(get_alibi_slopes(heads), dtype=np.float64)
    gen = torch.Generator().manual_seed(9900)
    done = torch.rand(9, 3, 1, generator=gen) < 0.3
    done[0, 0], done[-1, 1] = True, True
    q_segments, kv_segments = compute_segment_ids(done, 4)
    out["segments/done"], out["segments/q"], out["segments/kv"] = np_(done), np_(q_segments), np_(kv_segments)
    np.savez_compressed(HERE / "causal_attention.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("causal_attention.npz:", len(out), "arrays,", (HERE / "causal_attention.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
