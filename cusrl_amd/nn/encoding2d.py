"""The 2-D positional encodings (counterpart of cusrl/nn/layer/encoding.py:11-106).  Each layer is one broadcast add of a
``[C, H, W]`` table onto ``[..., C, H, W]``; torch's own launch is already exactly that, so they get no kernel (DESIGN.md
"Depthwise convolution").  The sinusoidal table is built with the reference's operations in the reference's order: the same bits
on the CPU."""

from __future__ import annotations

import torch
from torch import Tensor, nn

__all__ = ["LearnablePositionalEncoding2D", "SinusoidalPositionalEncoding2D", "sinusoidal_positional_encoding_2d"]


def _axis_embedding(length: int, channels: int, base: float, device, dtype) -> Tensor:
    """``[length, channels]``: sin in the even columns, cos in the odd ones, of ``position / base^(2 i / channels)``."""
    positions = torch.arange(length, device=device, dtype=dtype).unsqueeze(1)
    divisors = torch.pow(torch.tensor(base, device=device, dtype=dtype), torch.arange(0, channels, 2, device=device, dtype=dtype) / channels)
    angles = positions / divisors
    embedding = torch.zeros(length, channels, device=device, dtype=dtype)
    embedding[:, 0::2] = torch.sin(angles)
    embedding[:, 1::2] = torch.cos(angles)
    return embedding


def sinusoidal_positional_encoding_2d(height: int, width: int, num_channels: int, *, base: float = 10000.0,
                                      device: torch.device | None = None, dtype: torch.dtype = torch.float32) -> Tensor:
    """``[H, W, C]``: the first half of the channels encodes the row, the second half the column."""
    if num_channels % 4 != 0:
        raise ValueError(f"'num_channels' must be divisible by 4 for 2D sinusoidal encoding; got {num_channels}")
    half = num_channels // 2
    pe = torch.zeros(height, width, num_channels, device=device, dtype=dtype)
    pe[:, :, :half] = _axis_embedding(height, half, base, device, dtype).unsqueeze(1).expand(height, width, half)
    pe[:, :, half:] = _axis_embedding(width, half, base, device, dtype).unsqueeze(0).expand(height, width, half)
    return pe


class SinusoidalPositionalEncoding2D(nn.Module):
    """Adds the sinusoidal table to ``[..., C, H, W]`` (``C`` divisible by 4).  ``requires_grad``: make the table learnable."""

    def __init__(self, num_channels: int, height: int, width: int, base: float = 10000.0, requires_grad: bool = False):
        super().__init__()
        pe = sinusoidal_positional_encoding_2d(height, width, num_channels, base=base).permute(2, 0, 1)
        self.pe = nn.Parameter(pe, requires_grad=requires_grad)

    def forward(self, x: Tensor) -> Tensor:
        return x + self.pe.type_as(x)


class LearnablePositionalEncoding2D(nn.Module):
    """Adds a learnable ``[C, H, W]`` table, drawn from a normal of standard deviation 0.02 truncated at +-2, to ``[..., C, H, W]``."""

    def __init__(self, num_channels: int, height: int, width: int):
        super().__init__()
        self.pe = nn.Parameter(torch.zeros(num_channels, height, width))
        nn.init.trunc_normal_(self.pe, std=0.02)

    def forward(self, x: Tensor) -> Tensor:
        return x + self.pe.type_as(x)
