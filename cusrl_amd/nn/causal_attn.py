"""Recurrent transformer modules (counterpart of cusrl/nn/module/causal_attn.py:49-402 and cusrl/nn/utils/attention.py:16-77):
causal sliding-window self-attention over a cache of the last ``window_size`` inputs, and the encoder layer built on it.  The
same constructors, attribute and sub-module names, memory dict and error text as the reference, so its state dicts load
strictly.  The projections are library GEMMs; the attention between them is ``ops.band_sdpa`` on the views the projections
leave — the band, the cache mask, the ``done`` segments and ALiBi live in the kernel, no mask tensor is built (DESIGN.md
"Causal sliding-window attention")."""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Literal

import torch
from torch import Tensor, nn

from cusrl_amd.nn.encoding import RotaryEmbedding
from cusrl_amd.nn.feedforward import FeedForward
from cusrl_amd.nn.gate import get_gate_cls
from cusrl_amd.nn.module import Module, ModuleFactory
from cusrl_amd.nn.recurrent import select_initial_memory
from cusrl_amd.nn.transformer import _TransformerLayer

__all__ = ["CausalMultiheadSelfAttention", "CausalTransformerEncoderLayer", "compute_segment_ids", "get_alibi_slopes"]


def get_alibi_slopes(nheads: int) -> list[float]:
    """Per-head ALiBi slopes ("Train Short, Test Long", Press et al., 2022): a geometric sequence for a power-of-two head
    count, and for any other count that of the power of two below it followed by every other slope of the next one."""

    def power_of_2(n: int) -> list[float]:
        start = 2 ** (-(2 ** -(math.log2(n) - 3)))
        return [start * start**i for i in range(n)]

    if math.log2(nheads).is_integer():
        return power_of_2(nheads)
    closest = 2 ** math.floor(math.log2(nheads))
    return power_of_2(closest) + get_alibi_slopes(2 * closest)[0::2][: nheads - closest]


def compute_segment_ids(done: Tensor, window_size: int) -> tuple[Tensor, Tensor]:
    """``done [L, N, 1]`` -> int32 segment ids ``(q_segments [N, L], kv_segments [N, W + L])``: a step after a ``done`` opens a
    new segment, the ``W`` cache positions in front belong to segment 0."""
    done_t = done.squeeze(-1).transpose(0, 1)  # [N, L]
    shifted = torch.zeros(done_t.shape, dtype=done_t.dtype, device=done_t.device)
    shifted[:, 1:] = done_t[:, :-1]
    q_segments = shifted.cumsum(dim=1).to(torch.int32)
    kv_segments = done.new_zeros(done.size(1), done.size(0) + window_size, dtype=torch.int32)
    kv_segments[:, window_size:] = q_segments
    return q_segments, kv_segments


def _cache_survives(done: Tensor, window_size: int) -> Tensor:
    """bool ``[N, W]``: which of the last ``W`` steps still belong to the sequence open at the end of ``done [L, N, 1]`` — no
    ``done`` between the step and the last one (the reference's ``compute_reverse_cumulative_timesteps(done) == W - 1 - t``, which
    closes every sequence at the last row whatever ``done[-1]`` says)."""
    L, N = done.shape[:2]
    ends = done.new_zeros(window_size, N, dtype=torch.int32)
    steps = min(L, window_size)
    ends[window_size - steps:] = done[L - steps:].squeeze(-1)
    ends[-1] = 0
    return (ends.flip(0).cumsum(0).flip(0) == 0).transpose(0, 1)


@dataclass(slots=True)
class CausalMultiheadSelfAttentionFactory(ModuleFactory):
    embed_dim: int
    num_heads: int
    window_size: int
    dtype: torch.dtype = torch.float32
    alibi_slopes: Tensor | None = None
    rope_base: float | None = None

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        return CausalMultiheadSelfAttention(embed_dim=self.embed_dim, num_heads=self.num_heads, window_size=self.window_size,
                                            dtype=self.dtype, alibi_slopes=self.alibi_slopes, rope_base=self.rope_base,
                                            input_dim=input_dim, output_dim=output_dim)


class CausalMultiheadSelfAttention(Module):
    """Self-attention of ``input [L, N, ..., C]`` in which step ``t`` sees steps ``t - W ... t``, the ones in front of the input
    coming from the memory ``{"input_cache": [N, ..., W * C], "cache_mask": [N, ..., W]}`` (None: an empty cache), and no step
    sees across a ``done [L, N, 1]``.  Returns ``(output, memory)``, the memory holding the last ``W`` inputs."""

    Factory = CausalMultiheadSelfAttentionFactory

    def __init__(self, embed_dim: int, num_heads: int, window_size: int, dtype: torch.dtype = torch.float32,
                 alibi_slopes: Tensor | None = None, rope_base: float | None = None, input_dim: int | None = None,
                 output_dim: int | None = None):
        head_dim = embed_dim // num_heads
        if head_dim * num_heads != embed_dim:
            raise ValueError("'embed_dim' must be divisible by 'num_heads'")
        if rope_base is not None:
            if rope_base <= 0:
                raise ValueError("'rope_base' must be a positive number")
            if head_dim % 2 != 0:
                raise ValueError("'head_dim' must be even when RoPE is enabled")
        if alibi_slopes is not None:
            alibi_slopes = torch.as_tensor(alibi_slopes)
            if alibi_slopes.ndim != 1:
                raise ValueError("'alibi_slopes' must be a 1D tensor")
            if alibi_slopes.size(0) != num_heads:
                raise ValueError(f"'alibi_slopes' must contain {num_heads} elements")
        if window_size <= 0:
            raise ValueError("'window_size' must be a positive integer")
        super().__init__(input_dim=input_dim or embed_dim, output_dim=output_dim or embed_dim, is_recurrent=True)
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.window_size = window_size
        self.dtype = dtype
        self.rope_base = rope_base
        self.head_dim = head_dim

        self.q_proj = nn.Linear(self.input_dim, embed_dim)
        self.kv_proj = nn.Linear(self.input_dim, embed_dim * 2)
        self.out_proj = nn.Linear(embed_dim, self.output_dim)
        self.register_buffer("alibi_slopes", alibi_slopes, persistent=False)
        self.rope = RotaryEmbedding(self.head_dim, base=rope_base) if rope_base is not None else None

    def forward(self, input: Tensor, memory=None, *, done: Tensor | None = None, sequential: bool = True, **kwargs):
        from cusrl_amd import ops

        W = self.window_size
        if seq_missing := (input.dim() == 2 or not sequential):
            input = input.unsqueeze(0)
        if sequential and input.dim() >= 3:
            memory = select_initial_memory(memory, input.shape[:-1])
        batch_dims = input.shape[1:-1]
        input = input.flatten(1, -2).transpose(0, 1)  # [N, L, C]
        batch_size, seq_len, _ = input.shape

        q = self.q_proj(input).view(batch_size, seq_len, self.num_heads, self.head_dim)
        if memory is None:
            input_cache = input.new_zeros(batch_size, W, self.input_dim)
            kv_mask = q.new_zeros(batch_size, seq_len + W, dtype=torch.bool)
            kv_mask[:, -seq_len:] = True
        else:
            input_cache = memory["input_cache"].reshape(batch_size, W, self.input_dim)
            cache_mask = memory["cache_mask"].reshape(batch_size, W)
            kv_mask = cache_mask.new_ones(batch_size, seq_len + W)
            kv_mask[:, :W] = cache_mask

        full_input = torch.cat([input_cache, input], dim=1)
        # (the cache's projection carries no gradient: the band's key-major pass starts at key W)
        kv = torch.cat([self.kv_proj(input_cache).detach(), self.kv_proj(input)], dim=1)
        k, v = kv.unflatten(-1, (2, self.num_heads, self.head_dim)).unbind(dim=-3)  # two views of the packed projection

        if done is not None and len(batch_dims) > 1:
            done = done.repeat_interleave(batch_size // batch_dims[0], dim=1)
        q_segments = compute_segment_ids(done, W)[0].contiguous() if done is not None else None

        if self.rope is not None:
            q = self.rope(q, offset=W)
            k = self.rope(k)

        attn_out = ops.band_sdpa(q.to(self.dtype), k.to(self.dtype), v.to(self.dtype), W, key_valid=kv_mask, q_segment=q_segments,
                                 alibi_slopes=self.alibi_slopes, key_grad_from=W)
        # (sequence first before the projection, not after: its output is then contiguous, which the fused add + LayerNorm behind
        # it in the layer asks for)
        output = self.out_proj(attn_out.type_as(input).flatten(-2).transpose(0, 1))  # [L, N, output_dim]

        new_input_cache = full_input[:, -W:].detach()
        new_cache_mask = kv_mask[:, -W:]
        if done is not None:
            new_cache_mask = new_cache_mask.logical_and(_cache_survives(done, W))

        output = output.unflatten(1, batch_dims)
        if seq_missing:
            output = output.squeeze(0)
        return output, {"input_cache": new_input_cache.reshape(*batch_dims, W * self.input_dim),
                        "cache_mask": new_cache_mask.reshape(*batch_dims, W)}

    def reset_memory(self, memory, done=None):
        """Empty the cache in place: all of it, or the entries ``done`` (a slice, or a bool ``[N, 1]``) selects."""
        if memory is None:
            return
        input_cache, cache_mask = memory["input_cache"], memory["cache_mask"]
        if done is None:
            input_cache.zero_()
            cache_mask.fill_(False)
        else:
            if isinstance(done, Tensor):
                done = done.squeeze(-1)
            input_cache[done] = 0.0
            cache_mask[done] = False


@dataclass(slots=True)
class CausalTransformerEncoderLayerFactory(ModuleFactory):
    embed_dim: int
    num_heads: int
    window_size: int
    feedforward_dim: int | None = None
    activation_fn: type[nn.Module] = nn.GELU
    dropout: float = 0.0
    dtype: torch.dtype = torch.float32
    gate_type: str | None = "residual"
    layer_norm: Literal[None, "pre", "post"] = "post"
    use_alibi: bool = False
    rope_base: float | None = None

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        return CausalTransformerEncoderLayer(
            embed_dim=self.embed_dim, num_heads=self.num_heads, window_size=self.window_size, feedforward_dim=self.feedforward_dim,
            activation_fn=self.activation_fn, dropout=self.dropout, dtype=self.dtype, gate_type=self.gate_type,
            layer_norm=self.layer_norm, use_alibi=self.use_alibi, rope_base=self.rope_base, input_dim=input_dim, output_dim=output_dim)


class CausalTransformerEncoderLayer(Module):
    """:class:`CausalMultiheadSelfAttention` and a feed-forward block, each merged into the stream by ``gate_type``'s gate, with
    a LayerNorm before (``"pre"``), after (``"post"``) or not at all (None); the memory is the attention's."""

    Factory = CausalTransformerEncoderLayerFactory

    def __init__(self, embed_dim: int, num_heads: int, window_size: int, feedforward_dim: int | None = None,
                 activation_fn: type[nn.Module] = nn.GELU, dropout: float = 0.0, dtype: torch.dtype = torch.float32,
                 gate_type: str | None = "residual", layer_norm: Literal[None, "pre", "post"] = "post", use_alibi: bool = False,
                 rope_base: float | None = None, input_dim: int | None = None, output_dim: int | None = None):
        gate_cls = get_gate_cls(gate_type)
        super().__init__(input_dim=input_dim or embed_dim, output_dim=output_dim or embed_dim, is_recurrent=True)
        self.embed_dim = embed_dim
        self.layer_norm = layer_norm

        self.in_proj: nn.Module = nn.Linear(self.input_dim, embed_dim) if self.input_dim != embed_dim else nn.Identity()
        self.norm1 = nn.LayerNorm(embed_dim)
        self.self_attn = CausalMultiheadSelfAttention(
            embed_dim=embed_dim, num_heads=num_heads, window_size=window_size, dtype=dtype, input_dim=embed_dim, output_dim=embed_dim,
            alibi_slopes=get_alibi_slopes(num_heads) if use_alibi else None, rope_base=rope_base)
        self.dropout1 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate1 = gate_cls(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.feedforward = FeedForward(input_dim=embed_dim, feedforward_dim=feedforward_dim, dropout=dropout, output_dim=embed_dim,
                                       activation_fn=activation_fn)
        self.dropout2 = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.gate2 = gate_cls(embed_dim)
        self.out_proj: nn.Module = nn.Linear(embed_dim, self.output_dim) if self.output_dim != embed_dim else nn.Identity()

    def forward(self, input: Tensor, memory=None, *, done: Tensor | None = None, sequential: bool = True, **kwargs):
        pre_norm, post_norm = _TransformerLayer._pre_norm, _TransformerLayer._post_norm
        input = self.in_proj(input)
        if self.layer_norm == "pre":
            attn_out, memory = self.self_attn(pre_norm(self.norm1, input), memory, done=done, sequential=sequential)
            input = self.gate1(input, self.dropout1(attn_out))
            input = self.gate2(input, self.dropout2(self.feedforward(pre_norm(self.norm2, input))))
        elif self.layer_norm == "post":
            attn_out, memory = self.self_attn(input, memory, done=done, sequential=sequential)
            input = post_norm(self.norm1, self.gate1, input, self.dropout1(attn_out))
            input = post_norm(self.norm2, self.gate2, input, self.dropout2(self.feedforward(input)))
        else:
            attn_out, memory = self.self_attn(input, memory, done=done, sequential=sequential)
            input = self.gate1(input, self.dropout1(attn_out))
            input = self.gate2(input, self.dropout2(self.feedforward(input)))
        return self.out_proj(input), memory

    def step_memory(self, input, memory=None, **kwargs):
        input = self.in_proj(input)
        if self.layer_norm == "pre":
            input = _TransformerLayer._pre_norm(self.norm1, input)
        return self.self_attn.step_memory(input, memory, **kwargs)

    def reset_memory(self, memory, done=None):
        self.self_attn.reset_memory(memory, done)
