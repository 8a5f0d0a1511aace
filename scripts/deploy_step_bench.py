"""One ``DeployedPolicy`` step against ``agent.act`` (deterministic, inference mode) of the same actor, on cuda:0.

For an MLP agent (48 -> 256 -> 128 -> 12, observation normalisation) and a one-layer GRU agent (hidden 256, normalisation) at
B = 1, 64 and 4096: both paths in one process, alternating window by window; a window is ``--calls`` back-to-back calls
between two device events after a warm-up; the median of ``--windows`` windows with min and max, in microseconds per step, and
the library launches one step makes (``_native.launch_counts``; GEMMs and torch's own copies are not in that census).

    python scripts/deploy_step_bench.py [--windows 9] [--calls 200] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import cusrl_amd as cusrl  # noqa: E402
from cusrl_amd import _native  # noqa: E402

DEVICE = "cuda:0"


def build(case: str, batch: int):
    if case == "mlp":
        factory = cusrl.preset.PpoAgentFactory(normalize_observation=True, device=DEVICE)
    else:
        factory = cusrl.preset.RecurrentPpoAgentFactory(rnn_type="GRU", actor_num_layers=1, actor_hidden_size=256, critic_num_layers=1,
                                                        critic_hidden_size=256, normalize_observation=True, empty_cuda_cache=False,
                                                        device=DEVICE)
    agent = factory(cusrl.template.environment.EnvironmentSpec(48, 12, device=DEVICE))
    observation = torch.randn(batch, 48, device=DEVICE)
    agent.act(observation)
    with tempfile.TemporaryDirectory() as directory:
        policy = cusrl.DeployedPolicy.load(agent.export(directory), map_location=DEVICE)
    agent.actor_memory = None
    agent.set_inference_mode(True, deterministic=True)
    return agent, policy, observation


def window(step, calls: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        step()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def launches(step) -> dict[str, int]:
    before = dict(_native.launch_counts)
    step()
    return {name: count - before.get(name, 0) for name, count in _native.launch_counts.items() if count != before.get(name, 0)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--windows", type=int, default=9)
    parser.add_argument("--calls", type=int, default=200)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    results = []
    for case in ("mlp", "gru"):
        for batch in (1, 64, 4096):
            agent, policy, observation = build(case, batch)
            steps = {"agent.act": lambda: agent.act(observation), "DeployedPolicy": lambda: policy(observation)}
            census = {name: launches(step) for name, step in steps.items()}
            for step in steps.values():  # warm-up
                window(step, args.calls)
            samples = {name: [] for name in steps}
            for _ in range(args.windows):  # alternating
                for name, step in steps.items():
                    samples[name].append(window(step, args.calls))
            row = {"case": case, "B": batch}
            for name, values in samples.items():
                row[name] = {"median_us": round(statistics.median(values), 2), "min_us": round(min(values), 2),
                             "max_us": round(max(values), 2), "library_launches": census[name]}
            results.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
