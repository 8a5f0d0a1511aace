"""What the attention tests of both kinds (and ``tests/golden/make_attention_golden.py``) share: the table of recorded module
cases, the operands of the kernel cases cut from the golden pool, the attention formulas of include/cusrl_hip.h evaluated on the
CPU — float64: the expectation; float32 as a tiled online softmax with ``lse`` and a backward from ``lse`` and delta: a
restatement of the kernels' algorithm that shows without a GPU that the bounds are reachable — and the assertions."""

from __future__ import annotations

import math

import numpy as np
import torch

BOUND = 1e-5  # the standing bound, relative to the largest entry
OWN, TILE = 16, 32  # csrc/attention.hip: rows a workgroup owns, rows of the streamed side per step
# (N, H, Lq, Lk, D): the issue's list, Lq / Lk of T - 1, T, T + 1 for both tile sizes, D of 3 and 4
KERNEL_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 6), (1, 2, 3, 3, 2), (2, 2, 33, 33, 24), (1, 2, 65, 130, 32), (2, 1, 17, 257, 64),
                 (1, 1, 129, 129, 128), (1, 2, 15, 31, 8), (1, 2, 16, 32, 8), (1, 2, 17, 33, 8), (2, 1, 31, 15, 5), (2, 1, 32, 16, 12),
                 (1, 1, 33, 17, 7), (2, 2, 9, 11, 3), (2, 2, 9, 11, 4)]
ROW_STRIDE = 7919
OFFSETS = {"q": 0, "k": 1201, "v": 2503, "dout": 1777, "bias": 3571, "keep": 523}
Q_SCALE = 1.5

# ---------------------------------------------------------------------------------------------------- recorded module cases
# name -> (class name, constructor arguments, {input name: shape}, {call argument: mask kind | bool | int})
# mask kinds: "bool" (Lq, Lk) with query row 2 fully masked; "float" (N, H, Lq, Lk) with a few -inf entries
# No case holds a parameter whose gradient is identically zero in exact arithmetic: a vector added to every key alike shifts each
# query's scores by one constant, which softmax ignores, so the gradient of a separate ``k_proj.bias`` without a key norm, and of
# a LayerNorm ``k_norm.bias`` without RoPE behind it, is the reference's own rounding noise (1e-7 of the neighbouring gradients)
# and "within 1e-5 of its largest entry" says nothing about it.  Hence ``bias=False`` on the norm-less ``MultiheadAttention``
# cases (the packed ``qkv_proj`` / ``kv_proj`` biases carry their query / value parts) and ``qk_norm="layer"`` recorded with RoPE.
N, LQ, LK = 2, 5, 4
MODULE_CASES = {
    "self/8x2/plain": ("MultiheadSelfAttention", dict(embed_dim=8, num_heads=2), {"input": (N, LQ, 8)}, {}),
    "self/8x2/causal": ("MultiheadSelfAttention", dict(embed_dim=8, num_heads=2), {"input": (N, LQ, 8)}, {"is_causal": True}),
    "self/8x2/bool": ("MultiheadSelfAttention", dict(embed_dim=8, num_heads=2), {"input": (N, LQ, 8)}, {"attn_mask": "bool"}),
    "self/6x3/plain": ("MultiheadSelfAttention", dict(embed_dim=6, num_heads=3), {"input": (N, LQ, 6)}, {}),
    "self/6x3/float": ("MultiheadSelfAttention", dict(embed_dim=6, num_heads=3), {"input": (N, LQ, 6)}, {"attn_mask": "float"}),
    "self/8x2/seq_first": ("MultiheadSelfAttention", dict(embed_dim=8, num_heads=2, batch_first=False), {"input": (LQ, N, 8)},
                           {"is_causal": True}),
    "self/8x2/rms": ("MultiheadSelfAttention", dict(embed_dim=8, num_heads=2, qk_norm="rms"), {"input": (N, LQ, 8)}, {}),
    "self/8x2/layer_rope": ("MultiheadSelfAttention", dict(embed_dim=8, num_heads=2, qk_norm="layer", rope_base=10000.0),
                            {"input": (N, LQ, 8)}, {"is_causal": True}),
    "self/6x3/rope": ("MultiheadSelfAttention", dict(embed_dim=6, num_heads=3, rope_base=10000.0, bias=False), {"input": (N, LQ, 6)}, {}),
    "mha/8x2/plain": ("MultiheadAttention", dict(embed_dim=8, num_heads=2, bias=False), {"q": (N, LQ, 8), "k": (N, LK, 8), "v": (N, LK, 8)}, {}),
    "mha/8x2/dims": ("MultiheadAttention", dict(embed_dim=8, num_heads=2, k_dim=5, v_dim=7, bias=False),
                     {"q": (N, LQ, 8), "k": (N, LK, 5), "v": (N, LK, 7)}, {"attn_mask": "bool"}),
    "mha/6x3/float": ("MultiheadAttention", dict(embed_dim=6, num_heads=3, qk_norm="rms"),
                      {"q": (N, LQ, 6), "k": (N, LK, 6), "v": (N, LK, 6)}, {"attn_mask": "float"}),
    "mha/8x2/seq_first": ("MultiheadAttention", dict(embed_dim=8, num_heads=2, batch_first=False, qk_norm="rms"),
                          {"q": (LQ, N, 8), "k": (LK, N, 8), "v": (LK, N, 8)}, {"is_causal": True}),
    "cross/8x2/plain": ("MultiheadCrossAttention", dict(embed_dim=8, num_heads=2), {"q": (N, LQ, 8), "kv": (N, LK, 8)}, {}),
    "cross/6x3/kv_dim": ("MultiheadCrossAttention", dict(embed_dim=6, num_heads=3, kv_dim=5, qk_norm="rms"),
                         {"q": (N, LQ, 6), "kv": (N, LK, 5)}, {"attn_mask": "bool"}),
    "cross/8x2/causal": ("MultiheadCrossAttention", dict(embed_dim=8, num_heads=2, qk_norm="rms"), {"q": (N, LQ, 8), "kv": (N, LK, 8)},
                         {"is_causal": True}),
    "cross/8x2/seq_first": ("MultiheadCrossAttention", dict(embed_dim=8, num_heads=2, batch_first=False),
                            {"q": (LQ, N, 8), "kv": (LK, N, 8)}, {"attn_mask": "float"}),
    "rope/offset": ("RotaryEmbedding", dict(head_dim=6, max_seq_len=4), {"x": (N, LQ, 3, 6)}, {"offset": 3}),
    "encoder/post_residual_layer": ("TransformerEncoderLayer",
                                    dict(embed_dim=8, num_heads=2, feedforward_dim=16, activation_fn="SwiGlu", input_dim=5, output_dim=3),
                                    {"input": (N, LQ, 5)}, {"is_causal": True}),
    "encoder/pre_gru_rms": ("TransformerEncoderLayer",
                            dict(embed_dim=8, num_heads=2, feedforward_dim=16, activation_fn="SwiGlu", input_dim=5, output_dim=3,
                                 gate_type="gru", block_norm="rms", block_norm_order="pre", rope_base=10000.0),
                            {"input": (N, LQ, 5)}, {"attn_mask": "bool"}),
    "encoder/post_highway_none": ("TransformerEncoderLayer",
                                  dict(embed_dim=8, num_heads=2, feedforward_dim=16, activation_fn="SwiGlu", input_dim=5, output_dim=3,
                                       gate_type="highway", block_norm=None),
                                  {"input": (N, LQ, 5)}, {}),
    "decoder/post_residual_layer": ("TransformerDecoderLayer", dict(embed_dim=8, num_heads=2, context_dim=5, feedforward_dim=16),
                                    {"target": (N, LQ, 8), "context": (N, LK, 5)}, {"target_is_causal": True}),
    "decoder/pre_output_layer": ("TransformerDecoderLayer",
                                 dict(embed_dim=8, num_heads=2, context_dim=5, feedforward_dim=16, gate_type="output",
                                      block_norm_order="pre", input_dim=6),
                                 {"target": (N, LQ, 6), "context": (N, LK, 5)}, {"context_attn_mask": "bool", "target_attn_mask": "float"}),
}


def build_module(namespace, name: str):
    """The recorded module from ``namespace``'s classes (this project's ``cusrl_amd.nn`` or the reference's ``cusrl.nn``)."""
    cls, kwargs, _, _ = MODULE_CASES[name]
    kwargs = dict(kwargs)
    if "activation_fn" in kwargs:
        kwargs["activation_fn"] = getattr(namespace, kwargs["activation_fn"])
    return getattr(namespace, cls)(**kwargs)


def mask_shape(name: str, argument: str, kind: str) -> tuple:
    """Shape of a recorded mask: ``(Lq, Lk)`` for ``"bool"``, ``(N, H, Lq, Lk)`` for ``"float"``."""
    cls, kwargs, _, _ = MODULE_CASES[name]
    Lk = LQ if cls == "MultiheadSelfAttention" or cls == "TransformerEncoderLayer" or argument == "target_attn_mask" else LK
    return (LQ, Lk) if kind == "bool" else (N, kwargs["num_heads"], LQ, Lk)


def make_mask(kind: str, shape: tuple, generator: torch.Generator) -> torch.Tensor:
    if kind == "bool":
        mask = torch.rand(shape, generator=generator) < 0.7
        mask[0, 0] = True
        mask[2] = False  # a fully masked query row
        return mask
    mask = torch.randn(shape, generator=generator)
    mask[..., 1, 0] = -math.inf
    mask[0, 0, 3, -1] = -math.inf
    return mask


def recorded_state(g, prefix: str) -> dict[str, torch.Tensor]:
    return {str(key): torch.from_numpy(g[prefix + "state/" + str(key)].copy()) for key in g[prefix + "state_keys"]}


def recorded_call(g, name: str):
    """``(inputs by name, call arguments, w)`` of a recorded case as CPU tensors."""
    _, _, shapes, call = MODULE_CASES[name]
    prefix = name + "/"
    inputs = {key: torch.from_numpy(g[prefix + "input/" + key].copy()) for key in shapes}
    arguments = {key: torch.from_numpy(g[prefix + "call/" + key].copy()) if isinstance(value, str) else value for key, value in call.items()}
    return inputs, arguments, torch.from_numpy(g[prefix + "w"].copy())


def run_module(module, inputs: dict, arguments: dict, w: torch.Tensor, device="cpu") -> dict:
    """``{"out", "grad_<input>", "grad/<parameter>"}`` of ``(module(*inputs, **arguments) * w).sum()``."""
    leaves = {name: value.to(device).requires_grad_(True) for name, value in inputs.items()}
    arguments = {key: value.to(device) if isinstance(value, torch.Tensor) else value for key, value in arguments.items()}
    output = module(*leaves.values(), **arguments)
    params = dict(module.named_parameters())
    wanted = [*leaves.values(), *params.values()]
    grads = torch.autograd.grad((output * w.to(device)).sum(), wanted, allow_unused=True)
    result = {"out": output.detach()}
    for key, leaf, grad in zip([*("grad_" + n for n in leaves), *("grad/" + n for n in params)], wanted, grads):
        result[key] = torch.zeros_like(leaf) if grad is None else grad
    return result


def relative_to_largest(candidate, reference) -> float:
    reference = reference.detach().cpu().numpy() if isinstance(reference, torch.Tensor) else reference
    reference = np.asarray(reference, dtype=np.float64)
    candidate = candidate.detach().cpu().numpy().astype(np.float64) if isinstance(candidate, torch.Tensor) else np.asarray(candidate, np.float64)
    assert candidate.shape == reference.shape, (candidate.shape, reference.shape)
    largest = np.abs(reference).max()
    if largest == 0:
        return float(np.abs(candidate).max())
    return float(np.abs(candidate - reference).max() / largest)


def assert_module_matches(label: str, got: dict, g, name: str) -> float:
    """Every recorded tensor within 1e-5 of its largest entry (exactly zero where the recorded tensor is)."""
    prefix = name + "/result/"
    recorded = {key[len(prefix):]: g[key] for key in g.files if key.startswith(prefix)}
    assert sorted(got) == sorted(recorded), (sorted(got), sorted(recorded))
    errors = {key: relative_to_largest(got[key], value) for key, value in recorded.items()}
    print(f"{label}: worst {max(errors.values()):.3e} of the largest entry over {len(errors)} tensors")
    for key, error in errors.items():
        assert np.isfinite(got[key].detach().cpu().numpy()).all(), f"{label} {key}: not finite"
        assert error <= BOUND, f"{label} {key}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
    return max(errors.values())


# ------------------------------------------------------------------------------------------------------- kernel operands
def cut(g, name: str, shape: tuple, scale: float = 1.0) -> torch.Tensor:
    """fp32 operand ``name`` of ``shape``: flat entry e of row r (the last dimension is the row) is
    ``scale * pool[(7919 r + e + offset) % P]``."""
    pool = g["kernel_pool"]
    rows, width = int(np.prod(shape[:-1])), shape[-1]
    index = (np.arange(rows)[:, None] * ROW_STRIDE + np.arange(width)[None, :] + OFFSETS[name]) % pool.size
    return torch.from_numpy(np.ascontiguousarray(np.float32(scale) * pool[index]).reshape(shape))


def kernel_case(g, shape: tuple, mask: str | None = None, mask_shape: tuple | None = None, masked_rows=()) -> dict:
    """``q`` (scaled by 1.5), ``k``, ``v``, ``dout`` in the ``[N, L, H, D]`` layout.  ``mask``: None, ``"causal"``, ``"bool"`` (keep
    where the pool draw is above -0.5) or ``"float"`` (the pool draw; -inf where it is below -1), of ``mask_shape`` (default
    ``(N, H, Lq, Lk)``); ``masked_rows``: query rows with every key masked."""
    N, H, Lq, Lk, D = shape
    case = {"q": cut(g, "q", (N, Lq, H, D), Q_SCALE), "k": cut(g, "k", (N, Lk, H, D)), "v": cut(g, "v", (N, Lk, H, D)),
            "dout": cut(g, "dout", (N, Lq, H, D)), "mask": None, "is_causal": mask == "causal"}
    if mask in ("bool", "float"):
        draw = cut(g, "keep" if mask == "bool" else "bias", mask_shape or (N, H, Lq, Lk))
        if mask == "bool":
            case["mask"] = draw > -0.5
            case["mask"][..., list(masked_rows), :] = False
        else:
            case["mask"] = torch.where(draw < -1.0, torch.full_like(draw, -math.inf), draw)
            case["mask"][..., list(masked_rows), :] = -math.inf
    return case


# --------------------------------------------------------------------------------------------------------- the formulas
def _scores(case: dict, dtype):
    """``s [N, H, Lq, Lk]`` with -inf where masked, and the operands in ``dtype``."""
    q, k, v, dout = (case[name].detach().cpu().to(dtype) for name in ("q", "k", "v", "dout"))
    N, Lq, H, D = q.shape
    Lk = k.shape[1]
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32).to(dtype)  # (the fp32 scale the launch passes)
    s = torch.einsum("nihd,njhd->nhij", q, k) * scale
    if case.get("is_causal"):
        visible = torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None]  # top-left aligned
        s = s.masked_fill(~visible, -math.inf)
    mask = case.get("mask")
    if mask is not None:
        mask = mask.detach().cpu().expand(N, H, Lq, Lk)
        s = s.masked_fill(~mask, -math.inf) if mask.dtype == torch.bool else s + mask.to(dtype)
    return s, q, k, v, dout, scale


def _backward_from_lse(s, lse, out, q, k, v, dout, scale) -> dict:
    dead = torch.isinf(lse) | torch.isinf(s)  # (exp(-inf - (-inf)) is never evaluated)
    p = torch.where(dead, torch.zeros_like(s), torch.exp(torch.where(dead, torch.zeros_like(s), s - lse)))
    delta = (dout * out).sum(-1).permute(0, 2, 1)[..., None]  # [N, H, Lq, 1]
    ds = p * (torch.einsum("nihd,njhd->nhij", dout, v) - delta) * scale
    return {"dq": torch.einsum("nhij,njhd->nihd", ds, k), "dk": torch.einsum("nhij,nihd->njhd", ds, q),
            "dv": torch.einsum("nhij,nihd->njhd", p, dout)}


def sdpa_formulas(case: dict, dtype=torch.float64) -> dict:
    """``out``, ``lse``, ``dq``, ``dk``, ``dv`` by the formulas of include/cusrl_hip.h as they stand, each step in ``dtype``."""
    s, q, k, v, dout, scale = _scores(case, dtype)
    top = s.amax(-1, keepdim=True)
    shifted = torch.where(torch.isinf(top), torch.full_like(s, -math.inf), s - torch.where(torch.isinf(top), torch.zeros_like(top), top))
    total = torch.exp(shifted).sum(-1, keepdim=True)
    lse = torch.where(total > 0, top + torch.log(total), torch.full_like(top, -math.inf))
    p = torch.where(total > 0, torch.exp(shifted) / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(s))
    out = torch.einsum("nhij,njhd->nihd", p, v)
    return {"out": out, "lse": lse[..., 0], **_backward_from_lse(s, lse, out, q, k, v, dout, scale)}


def sdpa_restatement(case: dict) -> dict:
    """The kernels' algorithm in CPU float32: key tiles of ``TILE`` with the running maximum ``m``, sum ``l`` and accumulator
    rescaled by ``exp(m - m_new)``; ``lse = m + log(l)``; the backward from ``lse`` and ``delta = rowsum(dout * out)``."""
    s, q, k, v, dout, scale = _scores(case, torch.float32)
    N, H, Lq, Lk = s.shape
    m = torch.full((N, H, Lq, 1), -math.inf)
    l = torch.zeros(N, H, Lq, 1)
    acc = torch.zeros(N, H, Lq, q.shape[-1])
    for k0 in range(0, Lk, TILE):
        tile = s[..., k0:k0 + TILE]
        m_new = torch.maximum(m, tile.amax(-1, keepdim=True))
        seen = ~torch.isinf(m_new)
        base = torch.where(seen, m_new, torch.zeros_like(m_new))
        alpha = torch.where(seen, torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(torch.where(torch.isinf(m), base, m) - base)),
                            torch.ones_like(m))
        p = torch.where(seen & ~torch.isinf(tile), torch.exp(torch.where(torch.isinf(tile), torch.zeros_like(tile), tile - base)),
                        torch.zeros_like(tile))
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + torch.einsum("nhij,njhd->nhid", p, v[:, k0:k0 + TILE])
        m = m_new
    alive = l > 0
    out = torch.where(alive, acc / torch.where(alive, l, torch.ones_like(l)), torch.zeros_like(acc)).permute(0, 2, 1, 3).contiguous()
    lse = torch.where(alive, m + torch.log(torch.where(alive, l, torch.ones_like(l))), torch.full_like(m, -math.inf))
    return {"out": out, "lse": lse[..., 0], **_backward_from_lse(s, lse, out, q, k, v, dout, scale)}


def rope_formulas(x, cos, sin, dout, dtype=torch.float64) -> dict:
    """``out = x cos + rotate_half(x) sin`` and ``dx = dout cos - rotate_half(dout sin)``; ``cos`` / ``sin``: ``[L, D / 2]``."""
    x, cos, sin, dout = (t.detach().cpu().to(dtype) for t in (x, cos, sin, dout))
    cos, sin = cos.repeat(1, 2).unsqueeze(-2), sin.repeat(1, 2).unsqueeze(-2)
    rotate = lambda t: torch.cat((-t.chunk(2, -1)[1], t.chunk(2, -1)[0]), -1)  # noqa: E731
    return {"out": x * cos + rotate(x) * sin, "dx": dout * cos - rotate(dout * sin)}


def zero_reference_bound(case: dict) -> float:
    """The absolute bound where the float64 gradient is identically zero (``Lk == 1``): 1e-5 max|dout| max|v| max|k| scale."""
    D = case["q"].shape[-1]
    return BOUND * float(case["dout"].abs().max()) * float(case["v"].abs().max()) * float(case["k"].abs().max()) / math.sqrt(D)


def assert_sdpa_matches(label: str, got: dict, want: dict, case: dict, names=("out", "dq", "dk", "dv")) -> dict:
    """``out``, ``dq``, ``dk``, ``dv`` each within 1e-5 of the float64 tensor's largest entry (the absolute bound of
    :func:`zero_reference_bound` where that tensor is identically zero); nothing NaN.  Prints and returns what was measured."""
    errors = {}
    for name in names:
        reference = want[name].detach().cpu().numpy().astype(np.float64)
        candidate = got[name].detach().cpu().numpy()
        assert candidate.dtype == np.float32 and candidate.shape == reference.shape, f"{label} {name}: {candidate.shape} {reference.shape}"
        assert np.isfinite(candidate).all(), f"{label} {name}: not finite"
        largest = np.abs(reference).max()
        if largest == 0:
            errors[name] = float(np.abs(candidate).max())
            assert errors[name] <= zero_reference_bound(case), f"{label} {name}: {errors[name]:.3e} against a zero tensor"
            errors[name] = 0.0 if errors[name] == 0 else errors[name] / zero_reference_bound(case) * BOUND
        else:
            errors[name] = float(np.abs(candidate - reference).max() / largest)
    print(f"{label}: " + ", ".join(f"{name} {error:.3e}" for name, error in errors.items()))
    for name, error in errors.items():
        assert error <= BOUND, f"{label} {name}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
    return errors
