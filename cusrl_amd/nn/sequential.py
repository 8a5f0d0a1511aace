"""A chain of backbones (counterpart of cusrl/nn/module/sequential.py:15-78): "MLP encoder -> GRU -> MLP", "input normalisation
-> MLP -> action denormalisation".  The reference's semantics throughout: recurrent layers keep their memory under the string
keys "0", "1", ... of one dict, keyword arguments (``done``, ``sequential``, ...) reach every layer, and every layer's output and
intermediate representations are published under ``"{i}/{ClassName}."``."""

from __future__ import annotations

from collections.abc import Iterable
from dataclasses import dataclass

from torch import nn

from cusrl_amd.nn.module import Module, ModuleFactory

__all__ = ["Sequential", "SequentialFactory"]


@dataclass(slots=True)
class SequentialFactory(ModuleFactory):
    factories: Iterable[ModuleFactory]
    hidden_dims: Iterable[int | None]

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        output_dims = list(self.hidden_dims) + [output_dim]
        layers = []
        for factory, output_dim in zip(self.factories, output_dims, strict=True):
            layer = factory(input_dim, output_dim)
            layers.append(layer)
            input_dim = layer.output_dim
        return Sequential(layers)


class Sequential(Module):
    """``Sequential(a, b, c)`` or ``Sequential([a, b, c])``.  It is not an ``Mlp``, so the one-launch inference path
    (``fused_inference_layers``) does not match it and acting goes through the layers."""

    Factory = SequentialFactory
    layers: nn.ModuleList

    def __init__(self, modules, *args):
        if args:
            assert isinstance(modules, Module)
            layers: list[Module] = [modules, *args]
        else:
            layers = [modules] if isinstance(modules, Module) else list(modules)
        super().__init__(input_dim=layers[0].input_dim, output_dim=layers[-1].output_dim,
                         is_recurrent=any(layer.is_recurrent for layer in layers))
        self.layers = nn.ModuleList(layers)
        # (Module.batch_invariant: a padded bootstrap bucket is allowed only if every layer allows it)
        self.batch_invariant = all(layer.batch_invariant for layer in layers)

    def forward(self, input, memory=None, **kwargs):
        final_memory = {}
        for i, layer in enumerate(self.layers):
            if layer.is_recurrent:
                layer_memory = None if memory is None else memory.get(str(i))
                input, layer_memory = layer(input, memory=layer_memory, **kwargs)
                if layer_memory is not None:
                    final_memory[str(i)] = layer_memory
            else:
                input = layer(input, **kwargs)

            prefix = f"{i}/{type(layer).__name__}"
            self.intermediate_repr[f"{prefix}.output"] = input
            self.intermediate_repr.update({f"{prefix}.{key}": value for key, value in layer.intermediate_repr.items()})
        return (input, final_memory) if self.is_recurrent else input

    def clear_intermediate_repr(self):
        super().clear_intermediate_repr()
        for layer in self.layers:
            layer.clear_intermediate_repr()

    def reset_memory(self, memory, done=None):
        if not self.is_recurrent or memory is None:
            return
        for i, layer in enumerate(self.layers):
            if layer.is_recurrent:
                layer.reset_memory(memory.get(str(i)), done)
