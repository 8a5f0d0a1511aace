"""GLU activations (counterpart of cusrl/nn/layer/activation.py:7-26): ``a * act(b)`` for the two halves of the input along
``dim``.  Subclasses of ``nn.GLU`` with its ``dim`` argument, as in the reference; a split along the last dimension is one launch
per direction with the halves read in place (``ops.glu``, DESIGN.md "Gates and GLU")."""

from __future__ import annotations

from torch import Tensor, nn

__all__ = ["GeGlu", "SwiGlu"]


class GeGlu(nn.GLU):
    """``a * GELU(b)``, the exact (erf) GELU."""

    def forward(self, input: Tensor) -> Tensor:
        from cusrl_amd import ops

        return ops.glu("geglu", input, self.dim)


class SwiGlu(nn.GLU):
    """``a * SiLU(b)``."""

    def forward(self, input: Tensor) -> Tensor:
        from cusrl_amd import ops

        return ops.glu("swiglu", input, self.dim)
