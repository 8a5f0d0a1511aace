"""Transformer encoder and decoder layers (counterpart of cusrl/nn/layer/transformer.py:69-402): the same constructors,
sub-module names and order of operations as the reference, so its state dicts load strictly.  Attention is ``ops.sdpa``, the
feed-forward block and the gates are this package's own, and where the gate is the plain residual and the block norm a
LayerNorm, add + norm is one ``ops.add_layer_norm`` launch (DESIGN.md "Attention")."""

from __future__ import annotations

from typing import Literal

from torch import Tensor, nn

from cusrl_amd.nn.attention import MultiheadCrossAttention, MultiheadSelfAttention, make_norm
from cusrl_amd.nn.feedforward import FeedForward
from cusrl_amd.nn.gate import ResidualGate, get_gate_cls

__all__ = ["TransformerDecoderLayer", "TransformerEncoderLayer"]


class _TransformerLayer(nn.Module):
    """The two ways a sub-layer's output ``y`` joins the stream ``x``."""

    block_norm_order: str

    def _projections(self, input_dim: int | None, output_dim: int | None) -> None:
        self.input_dim = input_dim or self.embed_dim
        self.output_dim = output_dim or self.embed_dim

    @staticmethod
    def _pre_norm(norm: nn.Module, x: Tensor) -> Tensor:
        """``norm(x)``; a LayerNorm through ``ops.add_layer_norm`` without a residual."""
        if type(norm) is nn.LayerNorm:
            from cusrl_amd import ops

            return ops.add_layer_norm(x, None, norm.weight, norm.bias, norm.eps)[1]
        return norm(x)

    @staticmethod
    def _post_norm(norm: nn.Module, gate: nn.Module, x: Tensor, y: Tensor) -> Tensor:
        """``norm(gate(x, y))``; residual add + LayerNorm as one ``ops.add_layer_norm`` call."""
        if type(gate) is ResidualGate and type(norm) is nn.LayerNorm:
            from cusrl_amd import ops

            return ops.add_layer_norm(x, y, norm.weight, norm.bias, norm.eps)[1]
        return norm(gate(x, y))


class TransformerEncoderLayer(_TransformerLayer):
    """Self-attention and feed-forward, each merged into the stream by ``gate_type``'s gate, with ``block_norm`` before
    (``"pre"``) or after (``"post"``) each; ``input_dim`` / ``output_dim`` other than ``embed_dim`` add a projection."""

    def __init__(self, embed_dim: int, num_heads: int, feedforward_dim: int | None = None, activation_fn: type[nn.Module] = nn.GELU,
                 rope_base: float | None = None, dropout: float = 0.0, batch_first: bool = True, gate_type: str | None = "residual",
                 qk_norm: Literal["rms", "layer"] | None = None, block_norm: Literal["rms", "layer"] | None = "layer",
                 block_norm_order: Literal["pre", "post"] = "post", input_dim: int | None = None, output_dim: int | None = None):
        super().__init__()
        self.embed_dim = embed_dim
        self._projections(input_dim, output_dim)
        self.block_norm_order = block_norm_order
        gate_cls = get_gate_cls(gate_type)

        self.in_proj: nn.Module = nn.Linear(self.input_dim, embed_dim) if self.input_dim != embed_dim else nn.Identity()
        self.norm1 = make_norm(block_norm, embed_dim)
        self.self_attn = MultiheadSelfAttention(embed_dim=embed_dim, num_heads=num_heads, rope_base=rope_base, qk_norm=qk_norm,
                                                dropout=dropout, batch_first=batch_first)
        self.dropout1 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate1 = gate_cls(embed_dim)
        self.norm2 = make_norm(block_norm, embed_dim)
        self.feedforward = FeedForward(input_dim=embed_dim, feedforward_dim=feedforward_dim, dropout=dropout, output_dim=embed_dim,
                                       activation_fn=activation_fn)
        self.dropout2 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate2 = gate_cls(embed_dim)
        self.out_proj: nn.Module = nn.Linear(embed_dim, self.output_dim) if self.output_dim != embed_dim else nn.Identity()

    def forward(self, input: Tensor, attn_mask: Tensor | None = None, is_causal: bool = False) -> Tensor:
        input = self.in_proj(input)
        if self.block_norm_order == "pre":
            attn_out = self.self_attn(self._pre_norm(self.norm1, input), attn_mask=attn_mask, is_causal=is_causal)
            input = self.gate1(input, self.dropout1(attn_out))
            input = self.gate2(input, self.dropout2(self.feedforward(self._pre_norm(self.norm2, input))))
        else:
            attn_out = self.self_attn(input, attn_mask=attn_mask, is_causal=is_causal)
            input = self._post_norm(self.norm1, self.gate1, input, self.dropout1(attn_out))
            input = self._post_norm(self.norm2, self.gate2, input, self.dropout2(self.feedforward(input)))
        return self.out_proj(input)


class TransformerDecoderLayer(_TransformerLayer):
    """Self-attention over the target, cross-attention over a context ``[N, Lk, context_dim]`` and feed-forward, merged and
    normalised as in :class:`TransformerEncoderLayer`."""

    def __init__(self, embed_dim: int, num_heads: int, context_dim: int | None = None, feedforward_dim: int | None = None,
                 activation_fn: type[nn.Module] = nn.GELU, rope_base: float | None = None, dropout: float = 0.0,
                 batch_first: bool = True, gate_type: str | None = "residual", qk_norm: Literal["rms", "layer"] | None = None,
                 block_norm: Literal["rms", "layer"] | None = "layer", block_norm_order: Literal["pre", "post"] = "post",
                 input_dim: int | None = None, output_dim: int | None = None):
        super().__init__()
        self.embed_dim = embed_dim
        self.context_dim = context_dim or embed_dim
        self._projections(input_dim, output_dim)
        self.block_norm_order = block_norm_order
        gate_cls = get_gate_cls(gate_type)

        self.in_proj: nn.Module = nn.Linear(self.input_dim, embed_dim) if self.input_dim != embed_dim else nn.Identity()
        self.norm1 = make_norm(block_norm, embed_dim)
        self.self_attn = MultiheadSelfAttention(embed_dim=embed_dim, num_heads=num_heads, rope_base=rope_base, qk_norm=qk_norm,
                                                dropout=dropout, batch_first=batch_first)
        self.dropout1 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate1 = gate_cls(embed_dim)
        self.norm2 = make_norm(block_norm, embed_dim)
        self.cross_attn = MultiheadCrossAttention(embed_dim=embed_dim, num_heads=num_heads, qk_norm=qk_norm, dropout=dropout,
                                                  kv_dim=self.context_dim, batch_first=batch_first)
        self.dropout2 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate2 = gate_cls(embed_dim)
        self.norm3 = make_norm(block_norm, embed_dim)
        self.feedforward = FeedForward(input_dim=embed_dim, feedforward_dim=feedforward_dim, dropout=dropout, output_dim=embed_dim,
                                       activation_fn=activation_fn)
        self.dropout3 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate3 = gate_cls(embed_dim)
        self.out_proj: nn.Module = nn.Linear(embed_dim, self.output_dim) if self.output_dim != embed_dim else nn.Identity()

    def forward(self, target: Tensor, context: Tensor, target_attn_mask: Tensor | None = None,
                context_attn_mask: Tensor | None = None, target_is_causal: bool = False, context_is_causal: bool = False) -> Tensor:
        target = self.in_proj(target)
        if self.block_norm_order == "pre":
            attn_out = self.self_attn(self._pre_norm(self.norm1, target), attn_mask=target_attn_mask, is_causal=target_is_causal)
            target = self.gate1(target, self.dropout1(attn_out))
            attn_out = self.cross_attn(self._pre_norm(self.norm2, target), context, attn_mask=context_attn_mask,
                                       is_causal=context_is_causal)
            target = self.gate2(target, self.dropout2(attn_out))
            target = self.gate3(target, self.dropout3(self.feedforward(self._pre_norm(self.norm3, target))))
        else:
            attn_out = self.self_attn(target, attn_mask=target_attn_mask, is_causal=target_is_causal)
            target = self._post_norm(self.norm1, self.gate1, target, self.dropout1(attn_out))
            attn_out = self.cross_attn(target, context, attn_mask=context_attn_mask, is_causal=context_is_causal)
            target = self._post_norm(self.norm2, self.gate2, target, self.dropout2(attn_out))
            target = self._post_norm(self.norm3, self.gate3, target, self.dropout3(self.feedforward(target)))
        return self.out_proj(target)
