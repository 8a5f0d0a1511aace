#!/usr/bin/env python3
"""The fp32-MFMA attention forward (cusrl_sdpa_fwd_mfma) next to the VALU forward (cusrl_sdpa_fwd) on the same tensors: the
``[N, L, H, D]`` shapes below (``Lq = Lk = L``), causal and unmasked, and one line with a bool mask.  Each path is timed inside a
replayed graph of LAUNCHES launches (host clock around replays that end in a synchronise), the two alternating for ROUNDS rounds in
one process; a line gives the median of each in us per call, the spread (max - min) / median over the rounds, the rate over the
4 N H L^2 D operations of the two products (half of them under the causal mask) and the verdict: a path counts as faster only where
the ratio of the medians exceeds 1 + the larger of the two spreads.  The outputs of the two paths are compared first.
``--backward`` times cusrl_sdpa_bwd_mfma next to cusrl_sdpa_bwd instead (a call is both launches), on the same tensors with the
``out`` / ``lse`` of one cusrl_sdpa_fwd launch; the rate is over 10 N H L^2 D operations: the five distinct products s, dout . v, dq,
dk and dv at 2 N H L^2 D apiece, counted once each - the key-major pass computes s and dout . v a second time (seven MFMA products
in all, 14 N H L^2 D executed), and that recomputation is not counted as useful work.  It also prints each shape's causal /
unmasked time per path.
``--band`` times cusrl_band_sdpa_fwd_mfma next to cusrl_band_sdpa_fwd instead, through the ops' launch function on the same tensors:
``q [N, L, H, D]`` against the two slices of a packed ``[N, L + W, 2, H, D]`` projection, with a key-validity row, segment ids and
ALiBi slopes; the rate is over the 4 N H L (W + 1) D operations of the pairs inside the band.
``--band --backward`` times cusrl_band_sdpa_bwd_mfma next to cusrl_band_sdpa_bwd (a call is both launches) on those tensors with the
``out`` / ``lse`` of one cusrl_band_sdpa_fwd launch and ``key_grad_from = W`` (what nn/causal_attn.py passes with a detached cache),
plus one line with ``key_grad_from = 0``; the rate is over 10 N H L (W + 1) D operations, the five distinct products inside the band
counted once each as in ``--backward``.

    python scripts/sdpa_mfma_bench.py [--rounds 3] [--backward] [--band]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from cusrl_amd import ops  # noqa: E402
from cusrl_amd.ops.attention import _launch_sdpa_fwd, sdpa_backward  # noqa: E402
from cusrl_amd.ops.band_attention import _launch_band_fwd, band_sdpa_backward  # noqa: E402

SHAPES = ((256, 16, 4, 16), (64, 128, 4, 32), (16, 512, 8, 64), (4, 2048, 8, 128))  # [N, L, H, D]
CASES = [(shape, mask) for shape in SHAPES for mask in ("none", "causal")] + [((16, 512, 8, 64), "bool")]
# the band: the training shape of the causal transformer backbone at two batch sizes, then long sequences against the window
BAND_CASES = (((256, 24, 4, 16), 16), ((65536, 24, 4, 16), 16), ((64, 512, 8, 64), 64), ((16, 2048, 8, 128), 128))  # ([N, L, H, D], W)
LAUNCHES = 10


def captured(fn):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(LAUNCHES):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def replay_time(graph, seconds=0.2):
    """us per call over at least ``seconds`` of replays."""
    replays, elapsed = 0, 0.0
    t0 = time.perf_counter()
    while elapsed < seconds:
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        replays, elapsed = replays + 5, time.perf_counter() - t0
    return elapsed / replays / LAUNCHES * 1e6


def alternate(paths, rounds):
    """Median us per call and spread (max - min) / median of each path, the paths alternating within a round."""
    graphs = {path: captured(fn) for path, fn in paths.items()}
    times = {path: [] for path in paths}
    for _ in range(rounds):
        for path in paths:
            times[path].append(replay_time(graphs[path]))
    med = {path: statistics.median(times[path]) for path in paths}
    return med, {path: (max(times[path]) - min(times[path])) / med[path] for path in paths}


def band_backward(rounds, dev="cuda:0"):
    torch.manual_seed(0)
    for ((N, L, H, D), W), start in [(case, case[1]) for case in BAND_CASES] + [(BAND_CASES[0], 0)]:
        q, dout = torch.randn(N, L, H, D, device=dev), torch.randn(N, L, H, D, device=dev)
        k, v = torch.randn(N, L + W, 2, H, D, device=dev).unbind(dim=2)  # the slices of a packed projection, read where they are
        valid = torch.rand(N, L + W, device=dev) < 0.9
        valid[:, W:] = True  # (every query keeps its own token)
        segment = (torch.rand(N, L, device=dev) < 0.05).cumsum(1).int()
        slopes = torch.tensor([0.5 ** (h + 1) for h in range(H)], device=dev)
        assert ops.band_sdpa_bwd_mfma_supported(q, k, v, W, valid, segment, slopes, start)
        with torch.no_grad():
            out, lse = _launch_band_fwd(q, k, v, W, valid, segment, slopes, False)
            paths = {"mfma": lambda: band_sdpa_backward(q, k, v, out, lse, dout, W, valid, segment, slopes, start, matrix_core=True),
                     "valu": lambda: band_sdpa_backward(q, k, v, out, lse, dout, W, valid, segment, slopes, start)}
            before = ops._native.launch_counts.get("cusrl_band_sdpa_bwd_mfma", 0)
            got_m, got_v = paths["mfma"](), paths["valu"]()
            assert ops._native.launch_counts["cusrl_band_sdpa_bwd_mfma"] == before + 1
            differ = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got_m, got_v))
            del got_m, got_v
            med, spread = alternate(paths, rounds)
        ratio, noise = med["valu"] / med["mfma"], max(spread.values())
        verdict = "mfma faster" if ratio > 1 + noise else "valu faster" if 1 / ratio > 1 + noise else "within spread"
        flops = 10.0 * N * H * L * (W + 1) * D
        print(f"[{N:5d},{L:5d},{H:2d},{D:4d}] W {W:3d} from {start:3d}  mfma {med['mfma']:9.2f} us (spread {spread['mfma']:5.1%}, {flops / med['mfma'] / 1e6:6.2f} TFLOP/s)  "
              f"valu {med['valu']:9.2f} us (spread {spread['valu']:5.1%}, {flops / med['valu'] / 1e6:6.2f} TFLOP/s)  valu / mfma {ratio:5.2f}  {verdict}"
              f"  max |gradient difference| {differ:.1e} of the largest entry", flush=True)


def band(rounds, dev="cuda:0"):
    torch.manual_seed(0)
    for (N, L, H, D), W in BAND_CASES:
        q = torch.randn(N, L, H, D, device=dev)
        k, v = torch.randn(N, L + W, 2, H, D, device=dev).unbind(dim=2)  # the slices of a packed projection, read where they are
        valid = torch.rand(N, L + W, device=dev) < 0.9
        valid[:, W:] = True  # (every query keeps its own token)
        segment = (torch.rand(N, L, device=dev) < 0.05).cumsum(1).int()
        slopes = torch.tensor([0.5 ** (h + 1) for h in range(H)], device=dev)
        assert ops.band_sdpa_mfma_supported(q, k, v, W, valid, segment, slopes)
        paths = {"mfma": lambda: _launch_band_fwd(q, k, v, W, valid, segment, slopes, True),
                 "valu": lambda: _launch_band_fwd(q, k, v, W, valid, segment, slopes, False)}
        with torch.no_grad():
            before = ops._native.launch_counts.get("cusrl_band_sdpa_fwd_mfma", 0)
            (got_m, _), (got_v, _) = paths["mfma"](), paths["valu"]()
            assert ops._native.launch_counts["cusrl_band_sdpa_fwd_mfma"] == before + 1
            differ = float((got_m - got_v).abs().max() / got_v.abs().max())
            med, spread = alternate(paths, rounds)
        ratio, noise = med["valu"] / med["mfma"], max(spread.values())
        verdict = "mfma faster" if ratio > 1 + noise else "valu faster" if 1 / ratio > 1 + noise else "within spread"
        flops = 4.0 * N * H * L * (W + 1) * D
        print(f"[{N:5d},{L:5d},{H:2d},{D:4d}] W {W:3d}  mfma {med['mfma']:9.2f} us (spread {spread['mfma']:5.1%}, {flops / med['mfma'] / 1e6:6.2f} TFLOP/s)  "
              f"valu {med['valu']:9.2f} us (spread {spread['valu']:5.1%}, {flops / med['valu'] / 1e6:6.2f} TFLOP/s)  valu / mfma {ratio:5.2f}  {verdict}"
              f"  max |out difference| {differ:.1e} of the largest entry", flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--backward", action="store_true")
    parser.add_argument("--band", action="store_true")
    args = parser.parse_args()
    if args.band:
        return band_backward(args.rounds) if args.backward else band(args.rounds)
    rounds, unmasked = args.rounds, {}
    dev = "cuda:0"
    torch.manual_seed(0)
    for (N, L, H, D), kind in CASES:
        q, k, v = (torch.randn(N, L, H, D, device=dev) for _ in range(3))
        mask = torch.rand(L, L, device=dev) < 0.7 if kind == "bool" else None
        causal = kind == "causal"
        assert ops.sdpa_mfma_supported(q, k, v, mask, 0.0, causal)
        paths = {"mfma": lambda: _launch_sdpa_fwd(q, k, v, mask, causal, True), "valu": lambda: _launch_sdpa_fwd(q, k, v, mask, causal, False)}
        if args.backward:
            dout, (out, lse) = torch.randn(N, L, H, D, device=dev), paths["valu"]()
            before = ops._native.launch_counts.get("cusrl_sdpa_bwd_mfma", 0)
            paths = {"mfma": lambda: sdpa_backward(q, k, v, out, lse, dout, mask, causal, matrix_core=True),
                     "valu": lambda: sdpa_backward(q, k, v, out, lse, dout, mask, causal)}
        with torch.no_grad():
            got_m, got_v = paths["mfma"](), paths["valu"]()
            assert not args.backward or ops._native.launch_counts["cusrl_sdpa_bwd_mfma"] == before + 1
            differ = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got_m, got_v) if a.dim() == 4)
            med, spread = alternate(paths, rounds)
        ratio, noise = med["valu"] / med["mfma"], max(spread.values())
        verdict = "mfma faster" if ratio > 1 + noise else "valu faster" if 1 / ratio > 1 + noise else "within spread"
        flops = (10.0 if args.backward else 4.0) * N * H * L * L * D * (0.5 if causal else 1.0)
        print(f"[{N:3d},{L:5d},{H:2d},{D:4d}] {kind:6s}  mfma {med['mfma']:9.2f} us (spread {spread['mfma']:5.1%}, {flops / med['mfma'] / 1e6:6.2f} TFLOP/s)  "
              f"valu {med['valu']:9.2f} us (spread {spread['valu']:5.1%}, {flops / med['valu'] / 1e6:6.2f} TFLOP/s)  valu / mfma {ratio:5.2f}  {verdict}"
              f"  max |{'gradient' if args.backward else 'out'} difference| {differ:.1e} of the largest entry", flush=True)
        if kind == "none":
            unmasked = med
        elif kind == "causal":
            print(f"{'':20s} causal / unmasked: mfma {med['mfma'] / unmasked['mfma']:.2f}  valu {med['valu'] / unmasked['valu']:.2f}", flush=True)


if __name__ == "__main__":
    main()
