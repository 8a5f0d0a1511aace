"""Bijectors behind a policy's standard deviation (counterpart of cusrl/nn/layer/bijector.py:19-146).

Every class has a tensor form and a Python-float form of ``forward`` and ``inverse``.  The tensor forwards of the bounded
sigmoid and the bounded softplus are one HIP launch each way on the GPU (``ops.sigmoid_bijector`` / ``ops.softplus_bijector``,
cusrl_amd/csrc/bijector.hip); the inverses run once, when a distribution is constructed, and stay torch.

One known difference from the reference ("Std bijectors"): ``SoftplusBijector()`` and the bare spec ``"softplus"``
are the unbounded softplus here, while the reference clamps there with its defaults ``(1.0, 0.01, 1.0)``.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor, nn

__all__ = ["Bijector", "ExponentialBijector", "IdentityBijector", "SigmoidBijector", "SoftplusBijector", "make_bijector"]


class Bijector(nn.Module):
    @classmethod
    def from_str(cls, spec: str) -> "Bijector":
        """``cls(*params)`` for the ``_``-separated floats of ``spec`` (``""``: the defaults)."""
        return cls(*(float(param) for param in spec.split("_") if param))

    def forward(self, input):
        raise NotImplementedError

    def inverse(self, input):
        raise NotImplementedError


class IdentityBijector(Bijector):
    def forward(self, input):
        return input

    def inverse(self, input):
        return input


class ExponentialBijector(Bijector):
    def __init__(self, min_value: float = 0.01, max_value: float = 1.0):
        super().__init__()
        self.min_value, self.max_value = min_value, max_value
        self.min_input, self.max_input = math.log(min_value), math.log(max_value)

    def forward(self, input):
        if isinstance(input, Tensor):
            return torch.exp(input.clamp(self.min_input, self.max_input))
        return math.exp(min(max(input, self.min_input), self.max_input))

    def inverse(self, input):
        if isinstance(input, Tensor):
            return torch.log(input.clamp(self.min_value, self.max_value))
        return math.log(min(max(input, self.min_value), self.max_value))

    def extra_repr(self):
        return f"min={self.min_value}, max={self.max_value}"


class SigmoidBijector(Bijector):
    """``min_value + (max_value - min_value) * sigmoid(x)``; the inverse clamps to ``[min_value + eps, max_value - eps]``."""

    def __init__(self, min_value: float = 0.0, max_value: float = 1.0, eps: float = 0.01):
        super().__init__()
        self.min_value = min_value
        self.max_value = max_value
        self.range = max_value - min_value
        self.eps = eps

    def forward(self, input):
        if isinstance(input, Tensor):
            from cusrl_amd import ops

            return ops.sigmoid_bijector(input, self.min_value, self.max_value)
        return self.min_value + self.range * (1 / (1 + math.exp(-input)))

    def inverse(self, input):
        if isinstance(input, Tensor):
            clamped_input = input.clamp(self.min_value + self.eps, self.max_value - self.eps)
            return torch.log((clamped_input - self.min_value) / (self.max_value - clamped_input))
        clamped_input = max(self.min_value + self.eps, min(input, self.max_value - self.eps))
        return math.log((clamped_input - self.min_value) / (self.max_value - clamped_input))

    def extra_repr(self):
        return f"min={self.min_value}, max={self.max_value}, eps={self.eps}"


class SoftplusBijector(Bijector):
    """``softplus(clamp(x, min_input, max_input) * scale) / scale`` with ``min_input = inverse(min_value)`` and ``max_input =
    inverse(max_value)`` as soon as one of ``scale``, ``min_value``, ``max_value`` is given (the others take the reference's
    defaults ``1.0, 0.01, 1.0``); without any of them the plain, unbounded softplus."""

    def __init__(self, scale: float | None = None, min_value: float | None = None, max_value: float | None = None):
        super().__init__()
        self.bounded = not (scale is None and min_value is None and max_value is None)
        if not self.bounded:
            return
        self.scale = 1.0 if scale is None else scale
        self.min_value = 0.01 if min_value is None else min_value
        self.max_value = 1.0 if max_value is None else max_value
        self.min_input = self.inverse(self.min_value)
        self.max_input = self.inverse(self.max_value)

    def forward(self, input):
        if not self.bounded:
            if isinstance(input, Tensor):
                return nn.functional.softplus(input)
            return math.log1p(math.exp(input))
        if isinstance(input, Tensor):
            from cusrl_amd import ops

            return ops.softplus_bijector(input, self.scale, self.min_input, self.max_input)
        clamped_input = max(self.min_input, min(input, self.max_input))
        return math.log1p(math.exp(clamped_input * self.scale)) / self.scale

    def inverse(self, input):
        # log(exp(x) - 1) = x + log(1 - exp(-x))
        if not self.bounded:
            if isinstance(input, Tensor):
                return input + torch.log(-torch.expm1(-input))
            return input + math.log(-math.expm1(-input))
        if isinstance(input, Tensor):
            scaled = input.clamp(self.min_value, self.max_value) * self.scale
            return (scaled + torch.log1p(-torch.exp(-scaled))) / self.scale
        scaled = max(self.min_value, min(input, self.max_value)) * self.scale
        return (scaled + math.log1p(-math.exp(-scaled))) / self.scale

    def extra_repr(self):
        if not self.bounded:
            return "unbounded"
        return f"scale={self.scale}, min={self.min_value}, max={self.max_value}"


_BIJECTORS = {"": IdentityBijector, "identity": IdentityBijector, "exp": ExponentialBijector, "exponential": ExponentialBijector,
              "sigmoid": SigmoidBijector, "softplus": SoftplusBijector}


def make_bijector(spec) -> Bijector:
    """``None`` -> identity, an instance -> itself, ``"<type>[_<float>]*"`` -> ``<type>``'s class built from the floats; the type is
    case-insensitive, one of ``identity`` (or empty), ``exp`` / ``exponential``, ``sigmoid``, ``softplus``."""
    if spec is None:
        return IdentityBijector()
    if isinstance(spec, Bijector):
        return spec
    name, _, params = str(spec).partition("_")
    cls = _BIJECTORS.get(name.lower())
    if cls is None:
        raise ValueError(f"Unknown bijector '{spec}'")
    return cls.from_str(params)
