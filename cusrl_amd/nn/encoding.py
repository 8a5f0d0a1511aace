"""Rotary positional embedding (counterpart of ``RotaryEmbedding``, cusrl/nn/layer/encoding.py:128-198): the same constructor,
non-persistent ``inv_freq`` / ``cos_cached`` / ``sin_cached`` buffers, cache growth, ``offset`` and error text as the reference.
The rotation itself is one launch per direction (``ops.rope``, DESIGN.md "Attention")."""

from __future__ import annotations

import torch
from torch import Tensor, nn

__all__ = ["RotaryEmbedding"]


class RotaryEmbedding(nn.Module):
    """RoPE ("RoFormer: Enhanced Transformer with Rotary Position Embedding", https://arxiv.org/abs/2104.09864) over
    ``x [..., L, H, head_dim]``; ``head_dim`` even, the cache pre-built for ``max_seq_len`` positions and rebuilt when a longer
    sequence arrives."""

    inv_freq: Tensor
    cos_cached: Tensor
    sin_cached: Tensor

    def __init__(self, head_dim: int, max_seq_len: int = 2048, base: float = 10000.0):
        super().__init__()
        if head_dim % 2 != 0:
            raise ValueError("'head_dim' must be even to use rotary embeddings")
        self.head_dim = head_dim
        self.max_seq_len = int(max_seq_len)
        self.base = float(base)
        inv_freq = 1.0 / (self.base ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
        self.register_buffer("inv_freq", inv_freq, persistent=False)
        self.register_buffer("cos_cached", None, persistent=False)
        self.register_buffer("sin_cached", None, persistent=False)
        self._build_cache(self.max_seq_len)

    def _build_cache(self, seq_len: int) -> None:
        positions = torch.arange(seq_len, device=self.inv_freq.device, dtype=self.inv_freq.dtype)
        angles = positions.unsqueeze(1) @ self.inv_freq.unsqueeze(0)  # [L, head_dim / 2]
        self.cos_cached = torch.cos(angles)
        self.sin_cached = torch.sin(angles)

    def _get_cos_sin(self, seq_len: int, offset: int = 0, device: torch.device | None = None, dtype: torch.dtype | None = None):
        if offset < 0:
            raise ValueError("'offset' must be non-negative")
        end = offset + seq_len
        if end > self.cos_cached.shape[0]:
            self._build_cache(end)
        return (self.cos_cached[offset:end].to(device=device, dtype=dtype), self.sin_cached[offset:end].to(device=device, dtype=dtype))

    def forward(self, x: Tensor, offset: int = 0) -> Tensor:
        from cusrl_amd import ops

        cos, sin = self._get_cos_sin(x.shape[-3], offset=offset, device=x.device, dtype=x.dtype)
        return ops.rope(x, cos, sin)

    def apply_qkv(self, qkv: Tensor, offset: int = 0) -> Tensor:
        """``qkv [N, L, 3, H, head_dim]``: the queries and keys rotated, the values as they are."""
        q, k, v = qkv.unbind(dim=-3)
        return torch.stack([self(q, offset=offset), self(k, offset=offset), v], dim=-3)
