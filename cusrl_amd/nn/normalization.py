"""Fixed-statistics input normalisation and output denormalisation (counterpart of cusrl/nn/module/normalization.py:13-89):
the layers that usually sit at the two ends of a ``Sequential`` backbone.  Same constructors, error texts and state-dict keys
(``mean``, ``std``) as the reference; the per-column affine map is one launch (``ops.column_affine``, DESIGN.md "Column affine")."""

from __future__ import annotations

from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor, nn

from cusrl_amd.nn.module import Module, ModuleFactory

__all__ = ["Denormalization", "DenormalizationFactory", "Normalization", "NormalizationFactory"]


def _build(module_type, mean, std, input_dim: int | None, output_dim: int | None):
    module = module_type(torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32))
    if input_dim is not None and module.input_dim != input_dim:
        raise ValueError(f"Input dimension mismatch: expected {module.input_dim}, got {input_dim}")
    if output_dim is not None and module.output_dim != output_dim:
        raise ValueError(f"Output dimension mismatch: expected {module.output_dim}, got {output_dim}")
    return module


@dataclass(slots=True)
class NormalizationFactory(ModuleFactory):
    mean: Sequence[float] | np.ndarray | Tensor
    std: Sequence[float] | np.ndarray | Tensor

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        return _build(Normalization, self.mean, self.std, input_dim, output_dim)


class Normalization(Module):
    """``output = (input - mean) / std`` with ``mean`` and ``std`` given on construction and kept as non-trainable parameters."""

    Factory = NormalizationFactory
    inverse = False

    def __init__(self, mean: Tensor, std: Tensor):
        super().__init__(mean.size(0), mean.size(0))
        self.mean = nn.Parameter(mean, requires_grad=False)
        self.std = nn.Parameter(std, requires_grad=False)

    def forward(self, input: Tensor, **kwargs) -> Tensor:
        from cusrl_amd import ops

        # ([B, C] and temporal [T, B, C] batches alike: the launch sees [rows, C])
        return ops.column_affine(input, self.mean, self.std, inverse=self.inverse)


@dataclass(slots=True)
class DenormalizationFactory(ModuleFactory):
    mean: Sequence[float] | np.ndarray | Tensor
    std: Sequence[float] | np.ndarray | Tensor

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        return _build(Denormalization, self.mean, self.std, input_dim, output_dim)


class Denormalization(Normalization):
    """``output = input * std + mean``: the inverse of :class:`Normalization`."""

    Factory = DenormalizationFactory
    inverse = True
