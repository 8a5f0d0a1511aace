"""What the causal sliding-window attention tests of both kinds (and ``tests/golden/make_causal_attention_golden.py``) share: the
table of recorded module cases and how one is run, the kernel shapes and their side tensors, and the band formulas of
include/cusrl_hip.h evaluated in float64 on the CPU — written from the header, with a mask of its own (not the ops' builder)."""

from __future__ import annotations

import math

import torch

import _attention
from _attention import BOUND, assert_sdpa_matches, cut, relative_to_largest  # noqa: F401

# ---------------------------------------------------------------------------------------------------- recorded module cases
# name -> class, constructor arguments, input shape, warm-up length (None: no memory; the warm-up input is [warmup, *batch, C]),
# done as (step, env) pairs (None: no done), sequential, whether the memory is handed over sequence-aligned ([L, N, .], row 0
# the memory), and the input dimension C.
W = 4


def _case(cls, kwargs, shape, warmup=None, done=None, sequential=True, seq_memory=False):
    return dict(cls=cls, kwargs=kwargs, shape=shape, warmup=warmup, done=done, sequential=sequential, seq_memory=seq_memory)


def _attention_cases():
    cases = {}
    for E, H in ((8, 2), (6, 3)):
        base = dict(embed_dim=E, num_heads=H, window_size=W)
        tag = f"attn/{E}x{H}/"
        cases[tag + "no_memory"] = _case("CausalMultiheadSelfAttention", base, (5, 2, E))
        cases[tag + "short_warmup"] = _case("CausalMultiheadSelfAttention", base, (3, 2, E), warmup=2)              # L below W
        cases[tag + "done_first_last"] = _case("CausalMultiheadSelfAttention", base, (4, 2, E), warmup=3,            # L equal to W
                                               done=[(0, 0), (3, 0), (3, 1)])
        cases[tag + "done_consecutive"] = _case("CausalMultiheadSelfAttention", base, (7, 2, E), warmup=2,           # L above W
                                                done=[(2, 0), (3, 0), (5, 1)])
        cases[tag + "step_2d"] = _case("CausalMultiheadSelfAttention", base, (3, E), warmup=3)                       # L == 1, 2-D
        cases[tag + "not_sequential"] = _case("CausalMultiheadSelfAttention", base, (2, 3, E), warmup=2, sequential=False)
        cases[tag + "two_batch_dims_done"] = _case("CausalMultiheadSelfAttention", base, (5, 2, 3, E), warmup=3, done=[(1, 0), (4, 1)])
        cases[tag + "sequence_memory_done"] = _case("CausalMultiheadSelfAttention", base, (5, 2, E), warmup=2, done=[(2, 1)],
                                                    seq_memory=True)
        cases[tag + "rope"] = _case("CausalMultiheadSelfAttention", dict(base, rope_base=100.0), (6, 2, E), warmup=2, done=[(3, 0)])
        cases[tag + "alibi"] = _case("CausalMultiheadSelfAttention", dict(base, alibi_slopes=H), (6, 2, E), warmup=3, done=[(1, 1)])
        cases[tag + "rope_alibi"] = _case("CausalMultiheadSelfAttention", dict(base, alibi_slopes=H, rope_base=100.0), (5, 2, E), warmup=5)
        cases[tag + "dims"] = _case("CausalMultiheadSelfAttention", dict(base, input_dim=5, output_dim=3), (5, 2, 5), warmup=2,
                                    done=[(2, 0)])
    layer = dict(embed_dim=8, num_heads=2, window_size=W, feedforward_dim=16)
    cases["layer/post_residual"] = _case("CausalTransformerEncoderLayer", layer, (6, 2, 8), warmup=2, done=[(2, 0)])
    cases["layer/pre_gru"] = _case("CausalTransformerEncoderLayer", dict(layer, layer_norm="pre", gate_type="gru"), (6, 2, 8), warmup=2,
                                   done=[(3, 1)])
    cases["layer/none_highway"] = _case("CausalTransformerEncoderLayer", dict(layer, layer_norm=None, gate_type="highway"), (5, 2, 8),
                                        warmup=3)
    cases["layer/alibi_rope_dims"] = _case("CausalTransformerEncoderLayer",
                                           dict(layer, embed_dim=6, num_heads=3, use_alibi=True, rope_base=100.0, input_dim=5, output_dim=3),
                                           (6, 2, 5), warmup=2, done=[(0, 1), (4, 0)])
    return cases


MODULE_CASES = _attention_cases()


def build_module(namespace, name: str, get_alibi_slopes):
    """The recorded module from ``namespace``'s classes; an integer ``alibi_slopes`` stands for ``get_alibi_slopes`` of it."""
    case = MODULE_CASES[name]
    kwargs = dict(case["kwargs"])
    if "alibi_slopes" in kwargs:
        kwargs["alibi_slopes"] = torch.tensor(get_alibi_slopes(kwargs["alibi_slopes"]))
    return getattr(namespace, case["cls"])(**kwargs)


def make_inputs(name: str, generator: torch.Generator) -> dict:
    """``input``, ``warmup`` (when the case has a memory) and ``done`` (when it has one) of a case, drawn from ``generator``."""
    case = MODULE_CASES[name]
    shape = case["shape"]
    tensors = {"input": torch.randn(shape, generator=generator)}
    if case["warmup"] is not None:
        batch = shape[:-1] if not case["sequential"] or len(shape) == 2 else shape[1:-1]
        tensors["warmup"] = torch.randn((case["warmup"], *batch, shape[-1]), generator=generator)
    if case["done"] is not None:
        done = torch.zeros(shape[0], shape[1], 1, dtype=torch.bool)
        for step, env in case["done"]:
            done[step, env] = True
        tensors["done"] = done
    return tensors


def recorded_inputs(g, name: str) -> dict:
    prefix = name + "/input/"
    return {key[len(prefix):]: torch.from_numpy(g[key].copy()) for key in g.files if key.startswith(prefix)}


def run_case(module, name: str, tensors: dict, w: torch.Tensor | None, device="cpu") -> dict:
    """``out``, the two memory entries, and (with ``w``) the gradients of ``(out * w).sum()`` with respect to the input and every
    parameter.  The memory comes from a no-grad pass over the warm-up input."""
    case = MODULE_CASES[name]
    memory = None
    if "warmup" in tensors:
        with torch.no_grad():
            _, memory = module(tensors["warmup"].to(device), None)
        if case["seq_memory"]:
            length = case["shape"][0]
            memory = {key: torch.stack([value] + [torch.zeros_like(value)] * (length - 1)) for key, value in memory.items()}
    leaf = tensors["input"].to(device).requires_grad_(True)
    done = tensors["done"].to(device) if "done" in tensors else None
    output, new_memory = module(leaf, memory, done=done, sequential=case["sequential"])
    result = {"out": output.detach(), "memory/input_cache": new_memory["input_cache"].detach(), "memory/cache_mask": new_memory["cache_mask"]}
    if w is not None:
        params = dict(module.named_parameters())
        wanted = [leaf, *params.values()]
        grads = torch.autograd.grad((output * w.to(device)).sum(), wanted, allow_unused=True)
        for key, tensor, grad in zip(["grad_input", *("grad/" + n for n in params)], wanted, grads):
            result[key] = torch.zeros_like(tensor) if grad is None else grad
    return result


def cache_is_a_copy(name: str) -> bool:
    """Is the recorded cache a copy of recorded input rows?  Not where the layer computes what its attention sees — an
    ``in_proj`` GEMM or the pre-norm LayerNorm in front of it: those bits are the recording machine's BLAS and LayerNorm, and
    another CPU (or the device) rounds them differently."""
    kwargs = MODULE_CASES[name]["kwargs"]
    if MODULE_CASES[name]["cls"] == "CausalMultiheadSelfAttention":
        return True  # (the attention caches its own input whatever its width)
    return kwargs.get("layer_norm", "post") != "pre" and kwargs.get("input_dim", kwargs["embed_dim"]) == kwargs["embed_dim"]


def assert_case_matches(label: str, got: dict, g, name: str, cache_exact: bool = True) -> float:
    """The cache mask equal, the cache bit for bit (``cache_exact``; without it the cache stands under the bound like every other
    tensor: :func:`cache_is_a_copy`), every other recorded tensor within BOUND of its largest entry."""
    prefix = name + "/result/"
    recorded = {key[len(prefix):]: g[key] for key in g.files if key.startswith(prefix)}
    assert sorted(got) == sorted(recorded), (sorted(got), sorted(recorded))
    got = dict(got)
    for key in ("memory/input_cache", "memory/cache_mask") if cache_exact else ("memory/cache_mask",):
        mine = got.pop(key).cpu().numpy()
        theirs = recorded.pop(key)
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape and (mine == theirs).all(), f"{label} {key}"
    errors = {key: relative_to_largest(got[key], value) for key, value in recorded.items()}
    print(f"{label}: worst {max(errors.values()):.3e} of the largest entry over {len(errors)} tensors")
    for key, error in errors.items():
        assert torch.isfinite(got[key]).all(), f"{label} {key}: not finite"
        assert error <= BOUND, f"{label} {key}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
    return max(errors.values())


# ------------------------------------------------------------------------------------------------------- kernel operands
# (N, H, Lq, W, D): a single element; both tile sizes (16 owned rows, 32 streamed) on either side for Lq and W; both load
# widths (D % 4); the largest D; the step shape at W around the chunk of 16
KERNEL_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 6), (2, 2, 15, 3, 8), (2, 2, 16, 16, 8), (2, 2, 17, 33, 8), (1, 2, 33, 15, 12),
                 (1, 2, 40, 31, 4), (1, 2, 40, 32, 3), (1, 1, 17, 40, 128)]
STEP_SHAPES = [(3, 2, 1, 1, 8), (3, 2, 1, 15, 8), (3, 2, 1, 16, 6), (3, 2, 1, 17, 8), (2, 3, 1, 40, 12)]
OPTIONS = ["plain", "valid", "segments", "slopes", "all"]


def make_valid(N: int, Lq: int, window: int) -> torch.Tensor:
    """bool ``[N, Lq + W]`` with holes: every fifth key, the last cache key and — in sequence 0 — the first current key, the two
    sides of the cache / current boundary.  The one query of a step keeps its own token."""
    valid = torch.ones(N, Lq + window, dtype=torch.bool)
    valid[:, torch.arange(Lq + window) % 5 == 2] = False
    valid[:, window - 1] = False
    if Lq > 1:
        valid[0, window] = False
    else:
        valid[:, window] = True
    return valid


def make_segments(N: int, Lq: int) -> torch.Tensor:
    """int32 ``[N, Lq]``: the number of boundaries in front of each query, with boundaries after the first, a middle and the
    last position and after positions 15 and 16 (both sides of a 16-row edge); odd sequences keep only the edge ones."""
    done = torch.zeros(N, Lq, dtype=torch.bool)
    for t in (0, Lq // 2, Lq - 1, 15, 16):
        if t < Lq:
            done[0::2, t] = True
            if t in (15, 16):
                done[1::2, t] = True
    segments = torch.zeros(N, Lq, dtype=torch.int32)
    for i in range(1, Lq):
        segments[:, i] = segments[:, i - 1] + done[:, i - 1].int()
    return segments


def make_slopes(H: int) -> torch.Tensor:
    return torch.tensor([0.5 ** (h + 1) for h in range(H)], dtype=torch.float32)


def kernel_case(g, shape: tuple, option: str = "plain", key_grad_from: int = 0) -> dict:
    """``q`` (scaled by 1.5), ``k``, ``v``, ``dout`` cut from the pool of ``attention.npz`` and the side tensors of ``option``."""
    N, H, Lq, window, D = shape
    Lk = Lq + window
    return {"q": cut(g, "q", (N, Lq, H, D), _attention.Q_SCALE), "k": cut(g, "k", (N, Lk, H, D)), "v": cut(g, "v", (N, Lk, H, D)),
            "dout": cut(g, "dout", (N, Lq, H, D)), "window": window, "key_grad_from": key_grad_from,
            "key_valid": make_valid(N, Lq, window) if option in ("valid", "all") else None,
            "q_segment": make_segments(N, Lq) if option in ("segments", "all") else None,
            "alibi_slopes": make_slopes(H) if option in ("slopes", "all") else None}


# --------------------------------------------------------------------------------------------------------- the formulas
def band_visible(case: dict) -> torch.Tensor:
    """bool ``[N, Lq, Lk]``: key j visible to query i iff i <= j <= i + W, the key exists, and the segments agree (the cache is
    segment 0)."""
    N, Lq = case["q"].shape[:2]
    window = case["window"]
    visible = torch.zeros(N, Lq, Lq + window, dtype=torch.bool)
    for i in range(Lq):
        visible[:, i, i:i + window + 1] = True
    if case.get("key_valid") is not None:
        visible &= case["key_valid"].cpu().bool()[:, None, :]
    if case.get("q_segment") is not None:
        segment = case["q_segment"].cpu().long()
        kv_segment = torch.cat([torch.zeros(N, window, dtype=torch.long), segment], dim=1)
        visible &= segment[:, :, None] == kv_segment[:, None, :]
    return visible


def band_formulas(case: dict, dtype=torch.float64) -> dict:
    """``out``, ``lse``, ``dq``, ``dk``, ``dv`` (the last two from key ``key_grad_from`` on) by the formulas of
    include/cusrl_hip.h: s_ij = scale (q_i . k_j) - slope_h (i + W - j), -inf where not visible."""
    q, k, v, dout = (case[name].detach().cpu().to(dtype) for name in ("q", "k", "v", "dout"))
    N, Lq, H, D = q.shape
    window, Lk = case["window"], k.shape[1]
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32).to(dtype)  # (the fp32 scale the launch passes)
    s = torch.einsum("nihd,njhd->nhij", q, k) * scale
    if case.get("alibi_slopes") is not None:
        distance = (torch.arange(Lq)[:, None] + window - torch.arange(Lk)[None, :]).to(dtype)
        s = s - case["alibi_slopes"].cpu().to(dtype)[None, :, None, None] * distance
    s = s.masked_fill(~band_visible(case)[:, None], -math.inf)
    top = s.amax(-1, keepdim=True)
    dead = torch.isinf(top)
    shifted = torch.where(dead, torch.full_like(s, -math.inf), s - torch.where(dead, torch.zeros_like(top), top))
    total = torch.exp(shifted).sum(-1, keepdim=True)
    lse = torch.where(total > 0, top + torch.log(torch.where(total > 0, total, torch.ones_like(total))), torch.full_like(top, -math.inf))
    p = torch.where(total > 0, torch.exp(shifted) / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(s))
    out = torch.einsum("nhij,njhd->nihd", p, v)
    delta = (dout * out).sum(-1).permute(0, 2, 1)[..., None]
    ds = p * (torch.einsum("nihd,njhd->nhij", dout, v) - delta) * scale
    start = case.get("key_grad_from", 0)
    return {"out": out, "lse": lse[..., 0], "dq": torch.einsum("nhij,njhd->nihd", ds, k),
            "dk": torch.einsum("nhij,nihd->njhd", ds, q)[:, start:], "dv": torch.einsum("nhij,nihd->njhd", p, dout)[:, start:]}


def dense_equivalent(case: dict):
    """The band as what the dense kernel takes: a bool keep-mask ``[N, 1, Lq, Lk]``, or with slopes an fp32 ``[N, H, Lq, Lk]``
    bias with -inf — built from :func:`band_visible`."""
    visible = band_visible(case)
    if case.get("alibi_slopes") is None:
        return visible[:, None].contiguous()
    N, Lq, Lk = visible.shape
    distance = (torch.arange(Lq)[:, None] + case["window"] - torch.arange(Lk)[None, :]).float()
    bias = -case["alibi_slopes"].cpu()[None, :, None, None] * distance
    return bias.expand(N, -1, Lq, Lk).masked_fill(~visible[:, None], -math.inf).contiguous()
