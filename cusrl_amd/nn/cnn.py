"""A convolutional encoder around a list of layers (counterpart of cusrl/nn/module/cnn.py:13-108): same constructor, same
``layers.<i>.*`` state-dict keys, same handling of flat observations and of any number of leading batch dimensions.  The module
itself is reshaping; the kernels are its layers' (``SeparableConv2d`` runs the project's depthwise kernels, a plain
``nn.Conv2d`` or ``nn.MaxPool2d`` runs as torch runs it)."""

from __future__ import annotations

import math
from collections.abc import Callable, Iterable
from dataclasses import dataclass

import torch
from torch import nn

from cusrl_amd.nn.module import Module, ModuleFactory

__all__ = ["Cnn", "CnnFactory"]


@dataclass(slots=True)
class CnnFactory(ModuleFactory):
    layer_factories: Iterable[Callable[[], nn.Module]]
    input_shape: tuple[int, int] | tuple[int, int, int]
    input_flattened: bool = True
    flatten_output: bool = True

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        module = Cnn([factory() for factory in self.layer_factories], input_shape=self.input_shape,
                     input_flattened=self.input_flattened, flatten_output=self.flatten_output, output_dim=output_dim)
        if input_dim is not None and module.input_dim != input_dim:
            raise ValueError(f"Input dimension mismatch: expected {module.input_dim}, got {input_dim}")
        return module


class Cnn(Module):
    """``layers`` applied to images of ``input_shape`` ``(H, W)`` or ``(C, H, W)``.  ``input_flattened``: the input's last
    dimension is the flat image and is unflattened first.  ``flatten_output``: the ``[C', H', W']`` result is flattened;
    ``output_dim`` (which needs ``flatten_output``) appends a ``Linear`` onto the flattened features.  ``input_dim`` is the
    image's element count; ``output_dim`` is the feature count the layers produce for one image, or the ``Linear``'s width."""

    Factory = CnnFactory
    # library GEMMs and convolutions choose their kernel (and summation order) by the batch they are given: a row evaluated
    # inside a padded bucket can differ in its last bits from the same row evaluated alone
    batch_invariant = False

    def __init__(self, layers: Iterable[nn.Module | Module], input_shape: tuple[int, int] | tuple[int, int, int],
                 input_flattened: bool = True, flatten_output: bool = True, output_dim: int | None = None):
        layers = nn.Sequential(*layers)
        if len(input_shape) not in (2, 3):
            raise ValueError("'input_shape' must be 2D or 3D")
        if len(input_shape) == 2:
            input_shape = (1, *input_shape)  # (a missing channel dimension)
        # the feature count, from one pass over a zero image on the CPU (where the layers were built; nothing is launched)
        super().__init__(math.prod(input_shape), layers(torch.zeros(input_shape)).numel())
        self.input_shape = input_shape
        self.layers: nn.Sequential = layers
        self.input_flattened = input_flattened
        if output_dim is not None:
            if not flatten_output:
                raise ValueError("'flatten_output' must be True if 'output_dim' is set")
            self.layers.append(nn.Flatten(-3))  # [channel, y, x]
            self.layers.append(nn.Linear(self.output_dim, output_dim))
            self.output_dim = output_dim
        elif flatten_output:
            self.layers.append(nn.Flatten(-3))

    def forward(self, input: torch.Tensor, **kwargs) -> torch.Tensor:
        if self.input_flattened:
            input = input.unflatten(-1, self.input_shape)
        batch_dims = input.shape[:-3]
        if batch_dims:  # the layers see one batch dimension
            input = input.flatten(0, -4)
        output = self.layers(input)
        if batch_dims:
            output = output.unflatten(0, batch_dims)
        return output
