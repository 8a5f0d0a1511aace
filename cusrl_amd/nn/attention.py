"""Multi-head attention layers (counterpart of cusrl/nn/layer/mha.py:16-391): the same constructors, attribute and sub-module
names, initialisation and error text as the reference, so its state dicts load strictly.  The projections are library GEMMs and
``q_norm`` / ``k_norm`` torch's own layers; the attention between them is ``ops.sdpa`` on the ``[N, L, H, D]`` views the
projections leave — one launch per direction, no transpose and no copy in front of it (DESIGN.md "Attention")."""

from __future__ import annotations

from typing import Literal

from torch import Tensor, nn

from cusrl_amd.nn.encoding import RotaryEmbedding

__all__ = ["MultiheadAttention", "MultiheadCrossAttention", "MultiheadSelfAttention", "make_norm"]


def make_norm(norm: Literal["rms", "layer"] | None, head_dim: int) -> nn.Module:
    if norm is None:
        return nn.Identity()
    if norm == "rms":
        return nn.RMSNorm(head_dim, eps=1e-6)
    if norm == "layer":
        return nn.LayerNorm(head_dim, eps=1e-6)
    raise ValueError(f"Unsupported normalization type: {norm!r}")


class _Attention(nn.Module):
    """What the three layers share: the head split, ``out_proj`` and the call into ``ops.sdpa``."""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float, batch_first: bool):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError(f"'embed_dim' ({embed_dim}) must be divisible by 'num_heads' ({num_heads})")
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.dropout = dropout
        self.batch_first = batch_first

    def _reset(self, *projections: nn.Linear) -> None:
        for projection in projections:
            nn.init.xavier_uniform_(projection.weight)
            if projection.bias is not None:
                nn.init.constant_(projection.bias, 0.0)

    def _attend(self, q: Tensor, k: Tensor, v: Tensor, attn_mask: Tensor | None, is_causal: bool) -> Tensor:
        """``q``, ``k``, ``v``: ``[N, L, H, D]``, normalised and rotated; returns ``out_proj`` of the attention output."""
        from cusrl_amd import ops

        attn_out = ops.sdpa(q, k, v, attn_mask=attn_mask, dropout_p=self.dropout if self.training else 0.0, is_causal=is_causal)
        attn_out = self.out_proj(attn_out.flatten(-2, -1).type_as(q))
        return attn_out if self.batch_first else attn_out.transpose(0, 1)


class MultiheadAttention(_Attention):
    """Attention of ``q [N, Lq, C]`` over ``k [N, Lk, k_dim]`` and ``v [N, Lk, v_dim]`` (``[L, N, .]`` with
    ``batch_first=False``), one projection each; ``attn_mask``: ``(Lq, Lk)``, ``(N, 1, Lq, Lk)`` or ``(N, H, Lq, Lk)``."""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0, qk_norm: Literal["rms", "layer"] | None = None,
                 bias: bool = True, k_dim: int | None = None, v_dim: int | None = None, batch_first: bool = True):
        super().__init__(embed_dim, num_heads, dropout, batch_first)
        self.k_dim = embed_dim if k_dim is None else int(k_dim)
        self.v_dim = embed_dim if v_dim is None else int(v_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.k_proj = nn.Linear(self.k_dim, embed_dim, bias=bias)
        self.v_proj = nn.Linear(self.v_dim, embed_dim, bias=bias)
        self.q_norm = make_norm(qk_norm, self.head_dim)
        self.k_norm = make_norm(qk_norm, self.head_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self._reset(self.q_proj, self.k_proj, self.v_proj, self.out_proj)

    def forward(self, q: Tensor, k: Tensor, v: Tensor, attn_mask: Tensor | None = None, is_causal: bool = False) -> Tensor:
        if not self.batch_first:
            q, k, v = q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1)
        heads = (self.num_heads, self.head_dim)
        q = self.q_norm(self.q_proj(q).unflatten(-1, heads))
        k = self.k_norm(self.k_proj(k).unflatten(-1, heads))
        v = self.v_proj(v).unflatten(-1, heads)
        return self._attend(q, k, v, attn_mask, is_causal)


class MultiheadCrossAttention(_Attention):
    """Attention of ``q [N, Lq, C]`` over a context ``kv [N, Lk, kv_dim]``; keys and values come out of one projection and are
    read as the two slices of its ``[N, Lk, 2, H, D]`` output."""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0, qk_norm: Literal["rms", "layer"] | None = None,
                 bias: bool = True, kv_dim: int | None = None, batch_first: bool = True):
        super().__init__(embed_dim, num_heads, dropout, batch_first)
        self.kv_dim = embed_dim if kv_dim is None else int(kv_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.kv_proj = nn.Linear(self.kv_dim, 2 * embed_dim, bias=bias)
        self.q_norm = make_norm(qk_norm, self.head_dim)
        self.k_norm = make_norm(qk_norm, self.head_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self._reset(self.q_proj, self.kv_proj, self.out_proj)

    def forward(self, q: Tensor, kv: Tensor, attn_mask: Tensor | None = None, is_causal: bool = False) -> Tensor:
        if not self.batch_first:
            q, kv = q.transpose(0, 1), kv.transpose(0, 1)
        q = self.q_norm(self.q_proj(q).unflatten(-1, (self.num_heads, self.head_dim)))
        k, v = self.kv_proj(kv).unflatten(-1, (2, self.num_heads, self.head_dim)).unbind(dim=-3)
        return self._attend(q, self.k_norm(k), v, attn_mask, is_causal)


class MultiheadSelfAttention(_Attention):
    """Self-attention over ``input [N, L, C]``; queries, keys and values are the three slices of one projection's
    ``[N, L, 3, H, D]`` output.  ``rope_base``: rotary positions on queries and keys (``self.rope``), None for none."""

    def __init__(self, embed_dim: int, num_heads: int, rope_base: float | None = None, dropout: float = 0.0,
                 qk_norm: Literal["rms", "layer"] | None = None, bias: bool = True, batch_first: bool = True):
        super().__init__(embed_dim, num_heads, dropout, batch_first)
        self.rope_base = rope_base
        self.rope = RotaryEmbedding(self.head_dim, base=rope_base) if rope_base is not None else None
        self.qkv_proj = nn.Linear(embed_dim, 3 * embed_dim, bias=bias)
        self.q_norm = make_norm(qk_norm, self.head_dim)
        self.k_norm = make_norm(qk_norm, self.head_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self._reset(self.qkv_proj, self.out_proj)

    def forward(self, input: Tensor, attn_mask: Tensor | None = None, is_causal: bool = False) -> Tensor:
        if not self.batch_first:
            input = input.transpose(0, 1)
        q, k, v = self.qkv_proj(input).unflatten(-1, (3, self.num_heads, self.head_dim)).unbind(dim=-3)
        q, k = self.q_norm(q), self.k_norm(k)
        if self.rope is not None:
            q, k = self.rope(q), self.rope(k)
        return self._attend(q, k, v, attn_mask, is_causal)
