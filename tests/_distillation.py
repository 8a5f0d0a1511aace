"""Shared by the distillation tests (CPU and GPU): the experts and the agent of golden ``distillation.npz``
(tests/golden/make_distillation_golden.py), restated for this package."""

from __future__ import annotations

import torch
from torch import nn

ACTIVATIONS = ("ReLU", "ELU", "Tanh")
K, HIDDEN, A = 11, (32, 16), 3
LAYERS = len(HIDDEN) + 1
ENVS, STEPS, UPDATES = 16, 8, 3
TRACE_ACTIVATION = "ELU"
STUDENT_HIDDEN = (32, 16)


def tensors(g, activation):
    """``(weights, biases, mean, std, observation, output32, output64)`` of the fixture's expert, as CPU tensors."""
    p = f"expert/{activation}/"
    weights = [torch.from_numpy(g[f"{p}weight_{i}"]) for i in range(LAYERS)]
    biases = [torch.from_numpy(g[f"{p}bias_{i}"]) for i in range(LAYERS)]
    return (weights, biases, *(torch.from_numpy(g[p + name]) for name in ("mean", "std", "observation", "output32", "output64")))


def native_expert(cusrl, g, activation, device="cpu"):
    """The fixture's expert as an ``ExpertPolicy`` (the reference's ``Normalization`` does not clamp)."""
    weights, biases, mean, std, *_ = tensors(g, activation)
    return cusrl.ExpertPolicy(weights, biases, activation, mean=mean, std=std, clamp=None).to(device)


class Teacher(nn.Module):
    """``net((x - mean) / std)`` as a plain torch module: what the fixture's script scripted for the reference's hook."""

    def __init__(self, weights, biases, activation, mean, std):
        super().__init__()
        layers = []
        for i, (weight, bias) in enumerate(zip(weights, biases)):
            linear = nn.Linear(weight.shape[1], weight.shape[0])
            with torch.no_grad():
                linear.weight.copy_(weight)
                linear.bias.copy_(bias)
            layers.append(linear)
            if i + 1 < len(weights):
                layers.append(getattr(nn, activation)())
        self.net = nn.Sequential(*layers)
        self.register_buffer("mean", mean.clone())
        self.register_buffer("std", std.clone())

    def forward(self, observation: torch.Tensor) -> torch.Tensor:
        return self.net((observation - self.mean) / self.std)


def teacher(g, activation):
    weights, biases, mean, std, *_ = tensors(g, activation)
    return Teacher(weights, biases, activation, mean, std)


def scripted_expert_file(g, activation, directory) -> str:
    path = str(directory / f"expert_{activation}.pt")
    torch.jit.script(teacher(g, activation)).save(path)
    return path


def factory(cusrl, device, **overrides):
    """The fixture's agent: the `distillation` preset with 8 steps per update and a (32, 16) student; give it ``expert`` or
    ``expert_path``."""
    kwargs = dict(num_steps_per_update=STEPS, actor_hidden_dims=STUDENT_HIDDEN, device=device)
    kwargs.update(overrides)
    return cusrl.preset.DistillationAgentFactory(**kwargs)
