#!/usr/bin/env python3
"""One no-grad time step of a two-layer causal transformer (two ``CausalTransformerEncoderLayer``, post-norm, a full cache) inside
``ops.fused_attention_step()`` ("on": per layer one addmm, one cusrl_attn_step_forward launch, one addmm around the rest of the
layer) next to the same modules outside it ("off": the per-step chain with cusrl_band_sdpa_fwd), eager and as a replayed graph of
STEPS steps.  Host clock around windows that end in a synchronise, at least SECONDS each, the four variants alternating for
ROUNDS rounds in one process; a line gives the median of each in us per step and the largest spread (max - min) / median.  The
outputs and memories of the two ways are compared first.

    python scripts/attention_step_bench.py [--rounds 5] [--batches 64 1024 4096 16384]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from cusrl_amd import _native, nn, ops  # noqa: E402

MODELS = ((64, 4, 16), (128, 8, 32))  # (embed_dim, heads, window)
STEPS, SECONDS = 10, 0.2


def make_step(layers, x, memories, on):
    def step():
        with ops.fused_attention_step(on), torch.no_grad():
            hidden, out = x, []
            for layer, memory in zip(layers, memories):
                hidden, memory = layer(hidden, memory)
                out.append(memory)
            return hidden, out
    return step


def captured(step):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(STEPS):
            step()
    graph.replay()
    torch.cuda.synchronize()
    return graph.replay


def eager(step):
    def window():
        for _ in range(STEPS):
            step()
    return window


def window_time(window):
    """us per step over at least SECONDS of windows."""
    windows, elapsed = 0, 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while elapsed < SECONDS:
        for _ in range(5):
            window()
        torch.cuda.synchronize()
        windows, elapsed = windows + 5, time.perf_counter() - t0
    return elapsed / windows / STEPS * 1e6


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--batches", type=int, nargs="+", default=[64, 1024, 4096, 16384])
    args = parser.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    for E, H, W in MODELS:
        layers = [nn.CausalTransformerEncoderLayer(E, H, W).to(dev) for _ in range(2)]
        for N in args.batches:
            x = torch.randn(N, E, device=dev)
            memories = [{"input_cache": torch.randn(N, W * E, device=dev), "cache_mask": torch.rand(N, W, device=dev) < 0.9} for _ in layers]
            steps = {on: make_step(layers, x, memories, on) for on in (True, False)}
            before = _native.launch_counts.get("cusrl_attn_step_forward", 0)
            (out_on, mem_on), (out_off, mem_off) = steps[True](), steps[False]()
            assert _native.launch_counts.get("cusrl_attn_step_forward", 0) == before + 2
            assert all(torch.equal(a[key], b[key]) for a, b in zip(mem_on[:1], mem_off[:1]) for key in a)
            differ = float((out_on - out_off).abs().max() / out_off.abs().max())
            variants = {"eager on": eager(steps[True]), "eager off": eager(steps[False]),
                        "graph on": captured(steps[True]), "graph off": captured(steps[False])}
            for window in variants.values():
                window()   # warm
            times = {name: [] for name in variants}
            for _ in range(args.rounds):
                for name, window in variants.items():
                    times[name].append(window_time(window))
            med = {name: statistics.median(values) for name, values in times.items()}
            spread = max((max(values) - min(values)) / med[name] for name, values in times.items())
            print(f"E {E:3d} H {H} W {W:2d} N {N:5d}  " + "  ".join(f"{name} {med[name]:8.1f}" for name in variants) +
                  f" us/step  off / on: eager {med['eager off'] / med['eager on']:5.2f} graph {med['graph off'] / med['graph on']:5.2f}"
                  f"  spread {spread:5.1%}  max |out difference| {differ:.1e} of the largest entry", flush=True)


if __name__ == "__main__":
    main()
