"""Calling a module like a deployed policy (counterpart of cusrl/nn/module/inference.py:12-75).

``InferenceWrapper(module)`` keeps the recurrent ``memory`` between calls, takes NumPy arrays or tensors — one observation ``[C]``
or a batch ``[N, C]`` — and answers in the caller's container, device and dtype.  The forward runs without gradients on the
module's device, in the dtype of the module's parameters (a float64 NumPy observation is evaluated in fp32 and returned as
float64)."""

from __future__ import annotations

import functools
from typing import Any

import numpy as np
import torch

from cusrl_amd.nn.module import Module

__all__ = ["InferenceWrapper"]


def _preserve_io_format(forward):
    @functools.wraps(forward)
    def in_callers_format(self, input, **kwargs):
        is_numpy = isinstance(input, np.ndarray)
        tensor = torch.as_tensor(input)
        device, dtype = tensor.device, tensor.dtype
        compute = next((p.dtype for p in self.parameters() if p.is_floating_point()), dtype) if tensor.is_floating_point() else dtype
        output = forward(self, tensor.to(device=self.device, dtype=compute), **kwargs)
        output = output.to(device=device, dtype=dtype)
        return output.numpy() if is_numpy else output

    return in_callers_format


class InferenceWrapper(Module):
    def __init__(self, module: Module, memory: Any = None, forward_kwargs: dict[str, Any] | None = None):
        module = module.rnn_compatible()
        super().__init__(like=module, intermediate_repr=module.intermediate_repr)
        self._wrapped = module
        self.memory = memory
        self.forward_kwargs = forward_kwargs or {}

    @property
    def wrapped(self):
        return self._wrapped

    @_preserve_io_format
    @torch.no_grad()
    def forward(self, input: torch.Tensor, **kwargs):
        add_batch_dim = input.ndim == 1
        if add_batch_dim:
            input = input.unsqueeze(0)
        output, self.memory = self._wrapped(input, memory=self.memory, **self.forward_kwargs, **kwargs)
        if add_batch_dim:
            output = output.squeeze(0)
        return output

    def reset(self, indices=slice(None)):
        """Zero the carried memory of the given instances (all of them by default)."""
        self._wrapped.reset_memory(self.memory, indices)
