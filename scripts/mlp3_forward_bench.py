#!/usr/bin/env python3
"""The one-launch three-layer inference pass (cusrl_mlp3_forward) next to the library chain of the same module with
``fused_inference = False`` (four GEMMs, the activation launches, the sampling launch): every required width triple x {ELU, ReLU},
acting on 4096 rows with the sampling epilogue, 98 304 and 1 048 576 rows without.  Each pair is timed inside a replayed graph
and eagerly (host clock around work that ends in a synchronise), the two paths alternating for ROUNDS rounds in one process; a
line gives the median of each, the spread (max - min) / median over the rounds, and the verdict: the pass counts as faster only
where the ratio of the medians exceeds 1 + the larger of the two spreads.

    python scripts/mlp3_forward_bench.py [--rounds 3]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from cusrl_amd import ops  # noqa: E402
from cusrl_amd.nn import Actor, Mlp, NormalDist  # noqa: E402

TRIPLES = ((512, 256, 128), (256, 128, 64), (128, 128, 128))
CASES = ((4096, True, 20), (98304, False, 10), (1048576, False, 3))  # rows, sampling epilogue, launches per replay
K, A = 48, 12


def eager_time(fn, launches, replays=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches * replays):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replays / launches * 1e6


def captured(fn, launches):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(launches):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def replay_time(graph, launches, replays=5):
    t0 = time.perf_counter()
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replays / launches * 1e6


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    rounds = parser.parse_args().rounds
    dev = "cuda:0"
    torch.manual_seed(0)
    for widths in TRIPLES:
        for activation in ("ELU", "ReLU"):
            actor = Actor(Mlp(K, widths, activation_fn=activation, ends_with_activation=True), NormalDist(widths[-1], A)).to(dev)
            actor.fused_inference = False  # the module is the library chain; the pass is called directly
            layers = tuple(t.detach() for m in (*actor.backbone.layers[0::2], actor.distribution.mean_head) for t in (m.weight, m.bias))
            std = actor.distribution.std_vector()
            for rows, sample, launches in CASES:
                x, eps = torch.randn(rows, K, device=dev), torch.randn(rows, A, device=dev)

                def fused():
                    return ops.mlp3_forward(x, layers, activation, 1.0, std=std, eps=eps) if sample else ops.mlp3_forward(x, layers, activation)

                def chain():
                    return actor.explore(x) if sample else actor(x)

                with torch.no_grad():
                    graphs = {"fused": captured(fused, launches), "chain": captured(chain, launches)}
                    times = {(mode, path): [] for mode in ("graph", "eager") for path in ("fused", "chain")}
                    for _ in range(rounds):  # the two paths alternate within a round
                        for path, fn in (("fused", fused), ("chain", chain)):
                            times["graph", path].append(replay_time(graphs[path], launches))
                            times["eager", path].append(eager_time(fn, launches))
                flops = 2.0 * rows * (K * widths[0] + widths[0] * widths[1] + widths[1] * widths[2] + widths[2] * A)
                for mode in ("graph", "eager"):
                    med = {path: statistics.median(times[mode, path]) for path in ("fused", "chain")}
                    spread = {path: (max(times[mode, path]) - min(times[mode, path])) / med[path] for path in ("fused", "chain")}
                    ratio = med["chain"] / med["fused"]
                    verdict = "faster" if ratio > 1 + max(spread.values()) else "slower" if 1 / ratio > 1 + max(spread.values()) else "within spread"
                    print(f"{str(widths):16s} {activation:4s} rows {rows:8d} {'sampling' if sample else 'plain':8s} {mode:5s}  "
                          f"mlp3 {med['fused']:9.2f} us (spread {spread['fused']:5.1%}, {flops / med['fused'] / 1e6:6.1f} TFLOP/s)  "
                          f"chain {med['chain']:9.2f} us (spread {spread['chain']:5.1%})  chain / mlp3 {ratio:5.2f}  {verdict}", flush=True)
                del graphs


if __name__ == "__main__":
    main()
