"""The SimBa backbone (counterpart of cusrl/nn/module/simba.py:11-73): a residual pre-LayerNorm stack.  Same module tree and
state-dict keys as the reference; between its GEMMs every residual add runs fused with the LayerNorm behind it
(``ops.add_layer_norm``, DESIGN.md "Residual add + LayerNorm")."""

from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from cusrl_amd.nn.module import Linear, Module, ModuleFactory, linear_act, resolve_activation_fn

__all__ = ["Simba", "SimbaBlock", "SimbaFactory"]


@dataclass(slots=True)
class SimbaFactory(ModuleFactory):
    hidden_dim: int | None = None
    num_blocks: int = 1
    activation_fn: str | type[nn.Module] = "ReLU"

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        assert input_dim is not None
        return Simba(input_dim=input_dim, hidden_dim=self.hidden_dim, num_blocks=self.num_blocks, output_dim=output_dim,
                     activation_fn=self.activation_fn)


class SimbaBlock(nn.Sequential):
    """LayerNorm, Linear (H -> 4 H), activation, Linear (4 H -> H); ``forward`` adds the input back."""

    def __init__(self, hidden_dim: int, activation_fn: str | type[nn.Module] = "ReLU"):
        activation_fn = resolve_activation_fn(activation_fn)
        super().__init__(nn.LayerNorm(hidden_dim), Linear(hidden_dim, hidden_dim * 4), activation_fn(),
                         Linear(hidden_dim * 4, hidden_dim))

    def branch(self, normed: torch.Tensor) -> torch.Tensor:
        """What follows the block's LayerNorm; Linear -> ReLU as one GEMM with the ReLU in its epilogue, as in ``Mlp.forward``."""
        if type(self[2]) is nn.ReLU and normed.is_cuda and normed.dim() == 2:
            hidden = linear_act(normed, self[1].weight, self[1].bias, relu=True)
        else:
            hidden = self[2](self[1](normed))
        return self[3](hidden)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return input + super().forward(input)


class Simba(Module):
    """A network architecture described in "SimBa: Simplicity Bias for Scaling Up Parameters in Deep Reinforcement Learning",
    https://arxiv.org/abs/2410.09754.  ``hidden_dim=None``: no input projection, the width is ``input_dim``;
    ``output_dim=None``: no output projection."""

    Factory = SimbaFactory
    # the H -> 4 H -> H products of a no-grad pass are library GEMMs, whose kernel (and summation order) depends on the row count:
    # a few bootstrap rows evaluated inside a padded bucket differ in their last bits from the same rows evaluated alone
    batch_invariant = False

    def __init__(self, input_dim: int, hidden_dim: int | None = None, num_blocks: int = 1, output_dim: int | None = None,
                 activation_fn: str | type[nn.Module] = "ReLU"):
        self.hidden_dim = hidden_dim or input_dim
        super().__init__(input_dim, output_dim or self.hidden_dim)
        self.num_blocks = num_blocks

        self.blocks = nn.Sequential()
        if hidden_dim is not None:
            self.blocks.append(Linear(input_dim, self.hidden_dim))
        for _ in range(num_blocks):
            self.blocks.append(SimbaBlock(self.hidden_dim, activation_fn))
        self.blocks.append(nn.LayerNorm(self.hidden_dim))
        if output_dim is not None:
            self.blocks.append(Linear(self.hidden_dim, output_dim))

    def forward(self, input: torch.Tensor, **kwargs) -> torch.Tensor:
        from cusrl_amd import ops

        layers = list(self.blocks)
        x, i = input, 0
        if type(layers[0]) is Linear:
            x, i = layers[0](x), 1
        norms = [layer[0] if type(layer) is SimbaBlock else layer for layer in layers[i:i + self.num_blocks + 1]]
        if not (len(norms) == self.num_blocks + 1 and all(type(norm) is nn.LayerNorm for norm in norms)
                and ops.add_layer_norm_supported(x, None, norms[0].weight, norms[0].bias)):
            for layer in layers[i:]:  # (the rest of `self.blocks(input)`, exactly as the reference runs it)
                x = layer(x)
            return x
        # a plain LayerNorm in front of the first block; behind every block ONE pass adds its output to the residual stream and
        # normalises the sum for the next block (or for the output): num_blocks + 1 launches, no separate add
        stream, x = ops.add_layer_norm(x, None, norms[0].weight, norms[0].bias, norms[0].eps)
        for n in range(self.num_blocks):
            norm = norms[n + 1]
            stream, x = ops.add_layer_norm(layers[i + n].branch(x), stream, norm.weight, norm.bias, norm.eps)
        for layer in layers[i + self.num_blocks + 1:]:
            x = layer(x)
        return x
