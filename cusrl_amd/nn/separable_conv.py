"""Depthwise-separable 2-D convolution (counterpart of cusrl/nn/layer/separable_conv.py:7-85): the same two ``nn.Conv2d``
sub-modules, so the same state-dict keys, shapes and default initialisation.  On the device the depthwise half runs as the
project's own kernels (``ops.depthwise_conv2d``, DESIGN.md "Depthwise convolution") and the pointwise half as one batched GEMM."""

from __future__ import annotations

import torch
from torch import nn

__all__ = ["SeparableConv2d"]


class SeparableConv2d(nn.Module):
    """A spatial convolution applied to every input channel by itself (``depthwise``), then a ``1 x 1`` convolution that mixes
    the channels into ``out_channels`` (``pointwise``).  ``stride``, ``padding``, ``dilation`` and ``padding_mode`` belong to the
    depthwise half; ``bias`` to both."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int | tuple[int, int], stride: int | tuple[int, int] = 1,
                 padding: str | int | tuple[int, int] = 0, dilation: int | tuple[int, int] = 1, bias: bool = True,
                 padding_mode: str = "zeros", device: torch.device | str | None = None, dtype: torch.dtype | None = None):
        super().__init__()
        self.depthwise = nn.Conv2d(in_channels, in_channels, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation,
                                   groups=in_channels, bias=bias, padding_mode=padding_mode, device=device, dtype=dtype)
        self.pointwise = nn.Conv2d(in_channels, out_channels, kernel_size=1, bias=bias, device=device, dtype=dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from cusrl_amd import ops

        depthwise, pointwise = self.depthwise, self.pointwise
        if not ops.dwconv2d_supported(x, depthwise.weight, depthwise.bias, depthwise.stride, depthwise.padding, depthwise.dilation,
                                      depthwise.padding_mode):
            return pointwise(depthwise(x))  # (the reference's forward, as it is written there)
        hidden = ops.depthwise_conv2d(x, depthwise.weight, depthwise.bias, depthwise.stride, depthwise.padding, depthwise.dilation)
        # the 1 x 1 convolution is W [Co, C] @ hidden[n] [C, Ho Wo] for every image: one batched GEMM, then one in-place add of
        # the bias along the rows (two launches; autograd differentiates both)
        N, C, Ho, Wo = hidden.shape
        out = torch.bmm(pointwise.weight.view(1, -1, C).expand(N, -1, -1), hidden.view(N, C, Ho * Wo))
        if pointwise.bias is not None:
            out += pointwise.bias.view(-1, 1)
        return out.view(N, -1, Ho, Wo)
