"""The attention and rotary kernels and the attention / transformer modules on an MI355X: both attention entries through
``ops.Sdpa`` against the float64 formulas, masks in every broadcast form, fully masked rows, strided operands, memory safety,
reproducibility, error codes, the launch census, fallbacks, the reference's recorded runs (golden ``attention.npz``), RoPE, and
an agent whose actor runs a ``TransformerEncoderLayer``.

Worst figures measured on an MI355X over every kernel case (what DESIGN.md "Attention" quotes), relative to the float64 tensor's
largest entry: ``out`` 7.4e-7, ``dq`` 7.8e-7, ``dk`` 7.2e-7, ``dv`` 9.1e-7; RoPE 6.1e-8 both ways; modules against the recorded runs
at most 1.0e-6."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import _attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD, ROPE, LN_FWD, LN_BWD = "cusrl_sdpa_fwd", "cusrl_sdpa_bwd", "cusrl_rope_apply", "cusrl_add_layer_norm_fwd", "cusrl_add_layer_norm_bwd"
SYMBOLS = (FWD, BWD, ROPE, LN_FWD, LN_BWD)
GUARD = 64  # floats on either side of an operand (256 bytes: the operand keeps its 16-byte alignment)
SENTINEL = 12345.0
WORST: dict[str, float] = {}


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _counts():
    from cusrl_amd import _native

    return tuple(_native.launch_counts.get(symbol, 0) for symbol in SYMBOLS)


def _delta(before):
    return tuple(now - then for now, then in zip(_counts(), before))


def _sdpa(case, views=None) -> dict:
    """``out``, ``dq``, ``dk``, ``dv`` through ``ops.Sdpa``: one forward launch, one backward call.  ``views``: ready-made device
    leaves ``(q, k, v)`` (strided views of leaves of their own) in place of the case's contiguous tensors."""
    from cusrl_amd import ops

    mask = None if case["mask"] is None else case["mask"].to(DEV)
    q, k, v = views or (case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v"))
    assert ops.sdpa_supported(q, k, v, mask, 0.0, case["is_causal"])
    before = _counts()
    out = ops.sdpa(q, k, v, attn_mask=mask, is_causal=case["is_causal"])
    assert _delta(before)[:2] == (1, 0) and out.is_contiguous()
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case["dout"].to(DEV))
    assert _delta(before)[:2] == (1, 1)
    return {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}


def _record(errors: dict):
    for name, error in errors.items():
        WORST[name] = max(WORST.get(name, 0.0), error)


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("shape", _attention.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mask", [None, "causal"])
def test_kernels_match_the_float64_formulas(cusrl, golden, shape, mask):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    _record(_attention.assert_sdpa_matches(f"sdpa {shape} {mask}", _sdpa(case), _attention.sdpa_formulas(case), case))


def test_lse_is_the_rows_log_sum(cusrl, golden):
    from cusrl_amd.ops.attention import _launch_sdpa_fwd

    case = _attention.kernel_case(golden("attention"), (2, 2, 33, 70, 24), "float")
    _, lse = _launch_sdpa_fwd(*(case[n].to(DEV) for n in ("q", "k", "v")), case["mask"].to(DEV), False)
    assert _attention.relative_to_largest(lse, _attention.sdpa_formulas(case)["lse"]) <= _attention.BOUND


MASK_FORMS = {"LL": lambda N, H, Lq, Lk: (Lq, Lk), "N1LL": lambda N, H, Lq, Lk: (N, 1, Lq, Lk), "1HLL": lambda N, H, Lq, Lk: (1, H, Lq, Lk),
              "NHLL": lambda N, H, Lq, Lk: (N, H, Lq, Lk)}


@pytest.mark.parametrize("form", list(MASK_FORMS))
@pytest.mark.parametrize("kind", ["bool", "float"])
def test_masks_in_every_broadcast_form(cusrl, golden, kind, form):
    """Bool and float masks (the float one with -inf entries) with fully masked rows at the first, a middle and the last row and
    on both sides of the tile edges: those rows are exactly zero in ``out`` and ``dq``, nothing is NaN, the rest is in bound."""
    shape = (2, 3, 35, 40, 8)
    rows = [0, 15, 16, 31, 32, 34]
    case = _attention.kernel_case(golden("attention"), shape, kind, MASK_FORMS[form](*shape[:4]), masked_rows=rows)
    assert case["mask"].dim() == len(MASK_FORMS[form](*shape[:4]))
    if kind == "float":
        assert torch.isinf(case["mask"][..., 1, :]).any() and not torch.isinf(case["mask"][..., 1, :]).all()
    want, got = _attention.sdpa_formulas(case), _sdpa(case)
    _record(_attention.assert_sdpa_matches(f"sdpa {kind} mask {form}", got, want, case))
    assert not got["out"][:, rows].any() and not got["dq"][:, rows].any(), "a fully masked row is exactly zero"
    # the rows' contributions to dk and dv are exactly zero: the bits of the same call with those rows' dout zeroed
    without = dict(case, dout=case["dout"].clone())
    without["dout"][:, rows] = 0
    again = _sdpa(without)
    assert torch.equal(again["dk"], got["dk"]) and torch.equal(again["dv"], got["dv"])


def test_a_non_contiguous_mask(cusrl, golden):
    shape = (2, 2, 17, 33, 4)
    case = _attention.kernel_case(golden("attention"), shape, "bool", (2, 2, 33, 17))
    case["mask"] = case["mask"].transpose(-1, -2)  # (N, H, Lq, Lk), strides (.., 1, 17)
    assert not case["mask"].is_contiguous()
    strided = _sdpa(case)
    _record(_attention.assert_sdpa_matches("sdpa transposed mask", strided, _attention.sdpa_formulas(case), case))
    packed = _sdpa(dict(case, mask=case["mask"].contiguous()))
    assert all(torch.equal(strided[name], packed[name]) for name in strided)


# ------------------------------------------------------------------------------------------------- strided operands
@pytest.mark.parametrize("D", [8, 6])
def test_packed_and_transposed_views_launch_where_they_are(cusrl, golden, monkeypatch, D):
    """The slices of a packed ``[N, L, 3, H, D]`` / ``[N, L, 2, H, D]`` projection and the ``batch_first=False`` transposition are
    what the launch sees (their own data pointers and strides), and give the bits of their contiguous copies."""
    from cusrl_amd.ops import attention

    g = golden("attention")
    N, H, L = 2, 3, 19
    case = _attention.kernel_case(g, (N, H, L, L, D), "causal")
    seen = []
    real_fwd, real_bwd = attention._checked.cusrl_sdpa_fwd, attention._checked.cusrl_sdpa_bwd
    monkeypatch.setattr(attention._checked, "cusrl_sdpa_fwd", lambda *a: (seen.append(("fwd", a[:9])), real_fwd(*a))[1])
    monkeypatch.setattr(attention._checked, "cusrl_sdpa_bwd", lambda *a: (seen.append(("bwd", a[:9])), real_bwd(*a))[1])
    plain = _sdpa(case)
    seen.clear()

    qkv = torch.stack([case["q"], case["k"], case["v"]], dim=2).to(DEV).requires_grad_(True)  # [N, L, 3, H, D]
    q, k, v = qkv.unbind(dim=2)
    packed = _sdpa(case, (q, k, v))
    row = 3 * H * D
    for _, a in seen:
        assert a == (q.data_ptr(), L * row, row, k.data_ptr(), L * row, row, v.data_ptr(), L * row, row)
    assert (k.data_ptr() - q.data_ptr(), v.data_ptr() - q.data_ptr()) == (4 * H * D, 8 * H * D) and len(seen) == 2
    assert all(torch.equal(packed[name], plain[name]) for name in plain)
    seen.clear()

    kv = torch.stack([case["k"], case["v"]], dim=2).to(DEV).requires_grad_(True)
    k, v = kv.unbind(dim=2)
    q = case["q"].to(DEV).transpose(0, 1).contiguous().requires_grad_(True)  # [L, N, H, D]: batch_first=False
    mixed = _sdpa(case, (q.transpose(0, 1), k, v))
    for _, a in seen:
        assert a == (q.data_ptr(), H * D, N * H * D, k.data_ptr(), L * 2 * H * D, 2 * H * D, v.data_ptr(), L * 2 * H * D, 2 * H * D)
    assert len(seen) == 2 and all(torch.equal(mixed[name], plain[name]) for name in plain)


# ---------------------------------------------------------------------------------------------------- memory safety
class _Guarded:
    """A tensor inside a buffer with ``GUARD`` sentinel floats on either side."""

    def __init__(self, shape, values=None):
        numel = int(np.prod(shape))
        self.buffer = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.tensor = self.buffer[GUARD:GUARD + numel].view(shape)
        self.tensor.copy_(values) if values is not None else self.tensor.fill_(float("nan"))
        self.before = self.tensor.clone()
        assert self.tensor.data_ptr() % 16 == 0

    def guards_intact(self) -> bool:
        return bool((self.buffer[:GUARD] == SENTINEL).all() and (self.buffer[-GUARD:] == SENTINEL).all())

    def ptr(self):
        return self.tensor.data_ptr()


def _raw_calls(case, guarded: bool = True):
    """Both raw entries on guarded buffers: ``(status_fwd, status_bwd, inputs, outputs)``."""
    from cusrl_amd import _native

    lib = _native.lib()
    N, Lq, H, D = case["q"].shape
    Lk = case["k"].shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    ins = {name: _Guarded(case[name].shape, case[name].to(DEV)) for name in ("q", "k", "v", "dout")}
    outs = {"out": _Guarded((N, Lq, H, D)), "lse": _Guarded((N, H, Lq)), "dq": _Guarded((N, Lq, H, D)), "dk": _Guarded((N, Lk, H, D)),
            "dv": _Guarded((N, Lk, H, D)), "workspace": _Guarded((int(lib.cusrl_sdpa_bwd_workspace(N, H, Lq, Lk, D)),))}
    mask = None if case["mask"] is None else case["mask"].to(DEV)
    keep, bias = (mask if mask is not None and mask.dtype == torch.bool else None), (mask if mask is not None and mask.dtype != torch.bool else None)
    strides = (0, 0, 0, 0) if mask is None else mask.expand(N, H, Lq, Lk).stride()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rows = lambda L: (L * H * D, H * D)  # noqa: E731
    scale = 1.0 / math.sqrt(D)
    fwd = lib.cusrl_sdpa_fwd(ins["q"].ptr(), *rows(Lq), ins["k"].ptr(), *rows(Lk), ins["v"].ptr(), *rows(Lk), ptr(keep), ptr(bias), *strides,
                             int(case["is_causal"]), scale, outs["out"].ptr(), outs["lse"].ptr(), N, H, Lq, Lk, D, stream)
    bwd = lib.cusrl_sdpa_bwd(ins["q"].ptr(), *rows(Lq), ins["k"].ptr(), *rows(Lk), ins["v"].ptr(), *rows(Lk), outs["out"].ptr(), outs["lse"].ptr(),
                             ins["dout"].ptr(), *rows(Lq), ptr(keep), ptr(bias), *strides, int(case["is_causal"]), scale, outs["dq"].ptr(),
                             outs["dk"].ptr(), outs["dv"].ptr(), outs["workspace"].ptr(), N, H, Lq, Lk, D, stream)
    torch.cuda.synchronize()
    return fwd, bwd, ins, outs


@pytest.mark.parametrize("shape,mask", [((2, 3, 33, 47, 6), "causal"), ((2, 3, 33, 47, 8), "bool"), ((1, 2, 17, 16, 128), None),
                                        ((2, 1, 1, 1, 1), "float")])
def test_launches_stay_inside_their_operands(cusrl, golden, shape, mask):
    """Guard floats on both sides of every operand untouched, inputs unchanged, NaN-filled outputs fully written, on the 4-byte
    (D = 6, 1) and the 16-byte (D = 8, 128) path — and the bits of the autograd path."""
    case = _attention.kernel_case(golden("attention"), shape, mask)
    fwd, bwd, ins, outs = _raw_calls(case)
    assert (fwd, bwd) == (0, 0)
    for name, guarded in {**ins, **outs}.items():
        assert guarded.guards_intact(), name
        assert not torch.isnan(guarded.tensor).any(), f"{name}: not fully written"
    for name, guarded in ins.items():
        assert torch.equal(guarded.tensor, guarded.before), name
    expected = _sdpa(case)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(outs[name].tensor, expected[name]), name


@pytest.mark.parametrize("shape,mask", [((2, 2, 33, 33, 24), "causal"), ((1, 2, 65, 130, 32), None)])
def test_the_backward_gives_the_same_bits_every_time(cusrl, golden, shape, mask):
    case = _attention.kernel_case(golden("attention"), shape, mask)
    first, second = _sdpa(case), _sdpa(case)
    assert all(torch.equal(first[name], second[name]) for name in first)


def test_error_codes_on_the_device_write_nothing(cusrl, golden):
    from cusrl_amd import _native

    lib, invalid = _native.lib(), _native._CONSTANTS["E_INVALID"]
    stream = torch.cuda.current_stream().cuda_stream
    out = _Guarded((2, 3, 2, 4))
    t = torch.zeros(2, 3, 2, 4, device=DEV)
    p = t.data_ptr()
    lse = _Guarded((2, 2, 3))
    common = (p, 24, 8, p, 24, 8, p, 24, 8)
    assert lib.cusrl_sdpa_fwd(*common, p, p, 0, 0, 0, 0, 0, 0.5, out.ptr(), lse.ptr(), 2, 2, 3, 3, 4, stream) == invalid
    assert lib.cusrl_sdpa_fwd(*common, None, None, 0, 0, 0, 0, 0, 0.5, out.ptr(), lse.ptr(), 2, 2, 3, 3, 129, stream) == invalid
    assert lib.cusrl_sdpa_fwd(*common, None, None, 0, 0, 0, 0, 0, 0.5, out.ptr(), None, 2, 2, 3, 3, 4, stream) == invalid
    assert lib.cusrl_sdpa_fwd(*common, None, None, 0, 0, 0, 0, 0, 0.5, out.ptr(), lse.ptr(), 0, 2, 3, 3, 4, stream) == 0
    assert lib.cusrl_sdpa_bwd(*common, p, p, p, 24, 8, None, None, 0, 0, 0, 0, 0, 0.5, out.ptr(), out.ptr(), out.ptr(), None, 2, 2, 3, 3, 4,
                              stream) == invalid
    assert lib.cusrl_sdpa_bwd(*common, p, p, p, 24, 8, None, None, 0, 0, 0, 0, 0, 0.5, out.ptr(), out.ptr(), out.ptr(), lse.ptr(), 2, 2, -3, 3, 4,
                              stream) == invalid
    assert lib.cusrl_rope_apply(p, 24, 8, p, p, out.ptr(), 2, 3, 2, 3, 0, stream) == invalid
    assert lib.cusrl_rope_apply(p, 24, 8, p, None, out.ptr(), 2, 3, 2, 4, 0, stream) == invalid
    torch.cuda.synchronize()
    assert torch.isnan(out.tensor).all() and torch.isnan(lse.tensor).all() and out.guards_intact() and lse.guards_intact()


# ------------------------------------------------------------------------------------------------------------ census
def test_launch_census(cusrl):
    torch.manual_seed(5)
    x = torch.randn(3, 7, 8, device=DEV)
    for rope_base, ropes in ((None, 0), (10000.0, 2)):
        module = cusrl.MultiheadSelfAttention(8, 2, rope_base=rope_base).to(DEV)
        before = _counts()
        out = module(x.clone().requires_grad_(True), is_causal=True)
        assert _delta(before)[:3] == (1, 0, ropes)
        out.sum().backward()
        assert _delta(before)[:3] == (1, 1, 2 * ropes)
        before = _counts()
        with torch.no_grad():
            module(x)
        assert _delta(before)[:3] == (1, 0, ropes), "without a gradient: the forward launches alone"
    layer = cusrl.TransformerEncoderLayer(8, 2).to(DEV)
    before = _counts()
    out = layer(x.clone().requires_grad_(True))
    assert _delta(before) == (1, 0, 0, 2, 0)
    out.sum().backward()
    assert _delta(before) == (1, 1, 0, 2, 2)
    pre = cusrl.TransformerEncoderLayer(8, 2, block_norm_order="pre").to(DEV)
    before = _counts()
    pre(x.clone().requires_grad_(True)).sum().backward()
    assert _delta(before) == (1, 1, 0, 2, 2)


# --------------------------------------------------------------------------------------------------------- fallbacks
def test_fallbacks_launch_nothing_and_match_torch(cusrl, golden):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    sdpa = torch.nn.functional.scaled_dot_product_attention
    case = _attention.kernel_case(golden("attention"), (2, 3, 5, 7, 6), None)
    q, k, v = (case[n].to(DEV) for n in ("q", "k", "v"))
    want = sdpa(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
    before = _counts()
    assert torch.equal(ops.sdpa(q.double(), k.double(), v.double()), sdpa(*(t.double().transpose(1, 2) for t in (q, k, v))).transpose(1, 2))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not ops.sdpa_supported(q, k, v)
        assert torch.equal(ops.sdpa(q, k, v), sdpa(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2))
    wide = torch.randn(1, 3, 2, 130, device=DEV)
    assert torch.equal(ops.sdpa(wide, wide, wide), sdpa(*(wide.transpose(1, 2),) * 3).transpose(1, 2))
    module = cusrl.MultiheadSelfAttention(8, 2, dropout=0.5).to(DEV)
    x = torch.randn(2, 5, 8, device=DEV)
    module.train()
    assert torch.isfinite(module(x)).all()
    leaf = q.clone().requires_grad_(True)
    with double_differentiable():
        out = ops.sdpa(leaf, k, v)
        (grad,) = torch.autograd.grad(out.square().sum(), leaf, create_graph=True)
        (second,) = torch.autograd.grad(grad.square().sum(), leaf)
    assert torch.isfinite(second).all() and second.abs().max() > 0
    assert _delta(before) == (0, 0, 0, 0, 0)
    module.eval()
    module(x)
    assert _delta(before)[:2] == (1, 0), "the same module in eval() launches"
    assert _attention.relative_to_largest(ops.sdpa(q, k, v), want.double()) <= _attention.BOUND


# ---------------------------------------------------------------------------------------------------- recorded cases
@pytest.mark.parametrize("name", list(_attention.MODULE_CASES))
def test_module_reproduces_the_reference_on_the_device(cusrl, golden, name):
    g = golden("attention")
    module = _attention.build_module(cusrl.nn, name)
    module.load_state_dict(_attention.recorded_state(g, name + "/"), strict=True)
    inputs, arguments, w = _attention.recorded_call(g, name)
    before = _counts()
    got = _attention.run_module(module.to(DEV), inputs, arguments, w, device=DEV)
    launches = _delta(before)
    if name.startswith("rope"):
        assert launches[:3] == (0, 0, 2)
    else:
        attentions = 2 if name.startswith("decoder") else 1
        assert launches[:2] == (attentions, attentions), launches
    _record({"modules": _attention.assert_module_matches(name, got, g, name)})


# -------------------------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("D", [2, 6, 64])
def test_rope_matches_the_float64_formulas(cusrl, golden, D):
    from cusrl_amd import ops

    g = golden("attention")
    N, L, H = 3, 37, 5
    rope = cusrl.RotaryEmbedding(D, max_seq_len=16).to(DEV)
    x, dout = _attention.cut(g, "q", (N, L, H, D)), _attention.cut(g, "dout", (N, L, H, D))
    packed = torch.stack([x, x + 1], dim=2).to(DEV).requires_grad_(True)  # a strided view: slice 0 of [N, L, 2, H, D]
    view = packed.unbind(dim=2)[0]
    cos, sin = rope._get_cos_sin(L, offset=5, device=x.device, dtype=x.dtype)
    assert rope.cos_cached.shape[0] == L + 5 and ops.rope_supported(view, cos.to(DEV), sin.to(DEV))
    before = _counts()
    out = rope(view, offset=5)
    (grad,) = torch.autograd.grad(out, packed, dout.to(DEV))
    assert _delta(before)[2] == 2
    want = _attention.rope_formulas(x, cos, sin, dout)
    errors = {"rope out": _attention.relative_to_largest(out, want["out"]), "rope dx": _attention.relative_to_largest(grad[:, :, 0], want["dx"])}
    print(errors)
    _record(errors)
    assert max(errors.values()) <= _attention.BOUND and not grad[:, :, 1].any()
    assert torch.equal(rope(x.to(DEV), offset=5), out.detach()), "the view gives the bits of its contiguous copy"


# ------------------------------------------------------------------------------------------------------------ an agent
def test_agent_with_a_transformer_backbone_trains(cusrl):
    """The actor's backbone reshapes the observation to 4 tokens of 3 and runs a ``TransformerEncoderLayer`` in the eager ``ppo``
    preset: 8 envs, 4 steps per update, 2 epochs x 2 minibatches, 2 iterations."""

    class TokenBackbone(cusrl.Module):
        batch_invariant = False  # (library GEMMs: their summation order depends on the row count)

        def __init__(self, input_dim, tokens=4, embed_dim=8):
            super().__init__(input_dim, tokens * embed_dim)
            self.tokens = tokens
            self.layer = cusrl.TransformerEncoderLayer(embed_dim, 2, feedforward_dim=16, activation_fn=cusrl.SwiGlu, rope_base=10000.0,
                                                       input_dim=input_dim // tokens)

        def forward(self, input, **kwargs):
            tokens = input.reshape(-1, self.tokens, input.shape[-1] // self.tokens)
            return self.layer(tokens).reshape(*input.shape[:-1], -1)

    cusrl.set_global_seed(13)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=12, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=4, sampler_epochs=2, sampler_mini_batches=2).to_underlying()
    factory.actor_factory.backbone_factory = lambda input_dim, output_dim=None: TokenBackbone(input_dim)
    trainer = cusrl.Trainer(env, factory, num_iterations=3, verbose=False)
    agent = trainer.agent
    assert isinstance(agent.actor.backbone, TokenBackbone)
    initial = {name: param.detach().clone() for name, param in agent.named_parameters()}
    start = _counts()
    trainer.run_training_loop()
    torch.cuda.synchronize()
    fwd, bwd, rope, ln_fwd, ln_bwd = _delta(start)
    print(f"launches: sdpa fwd {fwd} bwd {bwd}, rope {rope}, add_layer_norm fwd {ln_fwd} bwd {ln_bwd}")
    assert fwd >= 3 * (4 + 4) and bwd >= 3 * 4 and rope >= 2 * fwd + 2 * bwd and ln_fwd >= 2 * fwd and ln_bwd >= 2 * bwd
    for key, value in trainer.last_info.items():
        if key.endswith("_loss"):
            assert np.isfinite(value), key
    assert np.isfinite(trainer.last_info["Agent/value_loss"])
    for name, param in agent.named_parameters():
        assert torch.isfinite(param).all(), name
        if param.requires_grad:
            assert not torch.equal(param, initial[name]), f"{name} did not change"


def test_worst_measured_errors_are_printed():
    print("worst measured, relative to the largest entry: " + ", ".join(f"{name} {error:.3e}" for name, error in sorted(WORST.items())))
    assert WORST and max(WORST.values()) <= _attention.BOUND
