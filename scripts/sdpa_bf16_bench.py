#!/usr/bin/env python3
"""The bf16 attention forward (cusrl_sdpa_fwd_bf16) next to the fp32-MFMA forward (cusrl_sdpa_fwd_mfma) on fp32 copies of the same
tensors and next to F.scaled_dot_product_attention on the same bf16 tensors: the ``[N, L, H, D]`` shapes of
scripts/sdpa_mfma_bench.py (``Lq = Lk = L``), unmasked and causal, timed by that script's method - each path inside a replayed graph
of LAUNCHES launches, host clock around replays that end in a synchronise, the three alternating for ROUNDS rounds in one process.
A line gives the median of each in us per call, the spread (max - min) / median over the rounds, the rate over the 4 N H L^2 D
operations of the two products (half of them under the causal mask) and the two ratios; a ratio counts as a difference only where it
exceeds 1 + the larger of the two spreads.  The bf16 output is first compared with the fp32 path's on the same (bf16-valued) operands.

    python scripts/sdpa_bf16_bench.py [--rounds 3]
"""
import argparse

import torch
from sdpa_mfma_bench import SHAPES, alternate  # (puts the repository root on sys.path)

from cusrl_amd import ops
from cusrl_amd.ops.attention import _launch_sdpa_fwd, _launch_sdpa_fwd_bf16, _sdpa_expression


def verdict(ratio, noise):
    return "faster" if ratio > 1 + noise else "slower" if 1 / ratio > 1 + noise else "within spread"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    rounds = parser.parse_args().rounds
    dev = "cuda:0"
    torch.manual_seed(0)
    for (N, L, H, D), causal in [(shape, causal) for shape in SHAPES for causal in (False, True)]:
        q, k, v = (torch.randn(N, L, H, D, device=dev).bfloat16() for _ in range(3))
        qf, kf, vf = q.float(), k.float(), v.float()
        assert ops.sdpa_bf16_supported(q, k, v, None, 0.0, causal) and ops.sdpa_mfma_supported(qf, kf, vf, None, 0.0, causal)
        paths = {"bf16": lambda: _launch_sdpa_fwd_bf16(q, k, v, None, causal), "fp32": lambda: _launch_sdpa_fwd(qf, kf, vf, None, causal, True),
                 "torch": lambda: _sdpa_expression(q, k, v, None, 0.0, causal)}
        with torch.no_grad():
            before = ops._native.launch_counts.get("cusrl_sdpa_fwd_bf16", 0)
            got, want = paths["bf16"]()[0], paths["fp32"]()[0]
            assert ops._native.launch_counts["cusrl_sdpa_fwd_bf16"] == before + 1
            differ = float((got.float() - want).abs().max() / want.abs().max())
            med, spread = alternate(paths, rounds)
        flops = 4.0 * N * H * L * L * D * (0.5 if causal else 1.0)
        text = "  ".join(f"{path} {med[path]:9.2f} us (spread {spread[path]:5.1%}, {flops / med[path] / 1e6:7.2f} TFLOP/s)" for path in paths)
        ratios = "  ".join(f"{other} / bf16 {med[other] / med['bf16']:5.2f} bf16 {verdict(med[other] / med['bf16'], max(spread[other], spread['bf16']))}"
                           for other in ("fp32", "torch"))
        print(f"[{N:3d},{L:5d},{H:2d},{D:4d}] {'causal' if causal else 'none':6s}  {text}  {ratios}"
              f"  max |out difference to fp32| {differ:.1e} of the largest entry", flush=True)


if __name__ == "__main__":
    main()
