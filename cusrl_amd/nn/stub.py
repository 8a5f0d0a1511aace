"""Placeholder modules (counterpart of cusrl/nn/module/stub.py:10-47): ``StubModule`` stands where an architecture needs a
module that computes nothing (the critic's backbone of the `distillation` preset), ``Identity`` hands its input through.  Same
constructors, asserts and outputs as the reference; neither launches a kernel of this package."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from cusrl_amd.nn.module import Module, ModuleFactory

__all__ = ["Identity", "IdentityFactory", "StubModule", "StubModuleFactory"]


@dataclass(slots=True)
class StubModuleFactory(ModuleFactory):
    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        assert input_dim is not None
        return StubModule(input_dim=input_dim, output_dim=output_dim)


class StubModule(Module):
    """A stub module serves as a placeholder in a model architecture."""

    Factory = StubModuleFactory

    def __init__(self, input_dim: int, output_dim: int | None):
        super().__init__(input_dim, output_dim or 1)

    def forward(self, input: torch.Tensor, **kwargs) -> torch.Tensor:
        return input.new_zeros((*input.shape[:-1], self.output_dim))


@dataclass(slots=True)
class IdentityFactory(ModuleFactory):
    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        assert input_dim is not None
        assert output_dim is None or output_dim == input_dim
        return Identity(input_dim=input_dim, output_dim=output_dim)


class Identity(Module):
    """An identity module that returns the input as is."""

    Factory = IdentityFactory

    def __init__(self, input_dim: int, output_dim: int | None):
        super().__init__(input_dim, output_dim or input_dim)
        assert self.input_dim == self.output_dim

    def forward(self, input: torch.Tensor, **kwargs) -> torch.Tensor:
        return input
