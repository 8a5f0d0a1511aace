"""The feed-forward block of a transformer layer (counterpart of ``FeedForward``, cusrl/nn/layer/transformer.py:12-66): Linear,
activation, optional dropout, Linear.  Same constructor and layer indices as the reference (state-dict keys ``layers.0.*`` and
``layers.2.*``, ``layers.3.*`` with dropout); with a GLU activation (``GeGlu`` / ``SwiGlu``) the second layer takes half the
feed-forward width."""

from __future__ import annotations

import torch
from torch import Tensor, nn

__all__ = ["FeedForward"]


class FeedForward(nn.Module):
    """``feedforward_dim`` defaults to ``4 * input_dim``, ``output_dim`` to ``input_dim``."""

    def __init__(self, input_dim: int, feedforward_dim: int | None = None, activation_fn: type[nn.Module] = nn.GELU,
                 dropout: float = 0.0, output_dim: int | None = None):
        super().__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim or input_dim
        self.feedforward_dim = feedforward_dim or input_dim * 4
        self.layers = nn.Sequential(nn.Linear(self.input_dim, self.feedforward_dim), activation_fn())
        if dropout > 0.0:
            self.layers.append(nn.Dropout(dropout))
        # the width the activation leaves (a GLU halves it), found by passing zeros through
        hidden_dim = self.layers(torch.zeros(1, self.input_dim)).size(-1)
        self.layers.append(nn.Linear(hidden_dim, self.output_dim))

    def forward(self, input: Tensor) -> Tensor:
        return self.layers(input)
