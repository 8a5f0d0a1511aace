"""Attention, the rotary embedding and the transformer layers without a GPU: the public surface, the reference's recorded state
dicts and runs (golden ``attention.npz``), the torch expression that CPU tensors take, what ``sdpa_supported`` refuses, the raw
entries' argument validation, and the kernels' algorithm restated in float32 against its float64 formulas under the assertions
the GPU tests use."""

from __future__ import annotations

import ctypes
import math

import pytest
import torch

import _attention

NAMES = ["MultiheadAttention", "MultiheadCrossAttention", "MultiheadSelfAttention", "RotaryEmbedding", "TransformerDecoderLayer",
         "TransformerEncoderLayer", "make_norm"]
SYMBOLS = {"cusrl_sdpa_fwd", "cusrl_sdpa_bwd", "cusrl_sdpa_bwd_workspace", "cusrl_rope_apply"}
OPS = ("sdpa", "sdpa_supported", "sdpa_backward", "Sdpa", "rope", "rope_supported", "Rope")


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def _launches():
    from cusrl_amd import _native

    return {symbol: _native.launch_counts.get(symbol, 0) for symbol in SYMBOLS}


def test_names_are_exported_from_both_namespaces(cusrl):
    import cusrl_amd.nn.attention
    import cusrl_amd.nn.encoding
    import cusrl_amd.nn.transformer
    from cusrl_amd import ops

    for namespace in (cusrl, cusrl.nn):
        assert set(NAMES) <= set(namespace.__all__)
        for name in NAMES:
            assert getattr(namespace, name) is getattr(cusrl.nn, name)
    assert set(cusrl.nn.attention.__all__) == {"MultiheadAttention", "MultiheadCrossAttention", "MultiheadSelfAttention", "make_norm"}
    assert cusrl.nn.encoding.__all__ == ["RotaryEmbedding"]
    assert set(cusrl.nn.transformer.__all__) == {"TransformerDecoderLayer", "TransformerEncoderLayer"}
    for name in OPS:
        assert hasattr(ops, name), name


def test_abi_stays_7_and_the_new_symbols_are_bound():
    from cusrl_amd import _native

    assert _native.ABI_VERSION == 7
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    assert _native._CONSTANTS["MAX_SDPA_HEAD_DIM"] == 128


def test_raw_entries_refuse_bad_arguments_without_a_gpu():
    """Argument validation runs on the host before anything is launched: every refusal is ``CUSRL_E_INVALID``."""
    from cusrl_amd import _native

    lib, invalid = _native.lib(), _native._CONSTANTS["E_INVALID"]
    a = 4096  # (a non-NULL address nothing dereferences: the entries return before a launch)
    sizes = dict(N=2, H=2, Lq=3, Lk=3, D=4)

    def fwd(q=a, k=a, v=a, keep=None, bias=None, out=a, lse=a, **changed):
        s = {**sizes, **changed}
        return lib.cusrl_sdpa_fwd(q, 24, 8, k, 24, 8, v, 24, 8, keep, bias, 0, 0, 0, 0, 0, 0.5, out, lse, s["N"], s["H"], s["Lq"], s["Lk"],
                                  s["D"], None)

    def bwd(q=a, k=a, v=a, out=a, lse=a, dout=a, keep=None, bias=None, dq=a, dk=a, dv=a, workspace=a, **changed):
        s = {**sizes, **changed}
        return lib.cusrl_sdpa_bwd(q, 24, 8, k, 24, 8, v, 24, 8, out, lse, dout, 24, 8, keep, bias, 0, 0, 0, 0, 0, 0.5, dq, dk, dv, workspace,
                                  s["N"], s["H"], s["Lq"], s["Lk"], s["D"], None)

    for name in ("q", "k", "v", "out", "lse"):
        assert fwd(**{name: None}) == invalid, name
    for name in ("q", "k", "v", "out", "lse", "dout", "dq", "dk", "dv", "workspace"):
        assert bwd(**{name: None}) == invalid, name
    for call in (fwd, bwd):
        assert call(keep=a, bias=a) == invalid, "a keep-mask and a bias in one call"
        for changed in (dict(N=-1), dict(H=0), dict(H=-1), dict(Lq=0), dict(Lk=-2), dict(D=0), dict(D=129), dict(D=-4)):
            assert call(**changed) == invalid, changed
        assert call(N=0) == 0, "N == 0 is a successful no-op"
    rope = lambda x=a, cos=a, sin=a, out=a, N=2, L=3, H=2, D=4, transpose=0: lib.cusrl_rope_apply(x, 24, 8, cos, sin, out, N, L, H, D,  # noqa: E731
                                                                                                  transpose, None)
    for changed in (dict(x=None), dict(cos=None), dict(sin=None), dict(out=None), dict(N=-1), dict(L=0), dict(H=0), dict(D=0), dict(D=3),
                    dict(transpose=2)):
        assert rope(**changed) == invalid, changed
    assert rope(N=0) == 0


def test_workspace_helper():
    from cusrl_amd import _native

    workspace = _native.lib().cusrl_sdpa_bwd_workspace
    assert workspace(2, 3, 5, 7, 6) == 2 * 3 * 5, "delta: one float per (n, h, query row)"
    assert workspace(1, 1, 1, 1, 1) == 1 and workspace(0, 2, 5, 7, 6) == 0
    assert workspace(4, 2, 129, 1, 128) == 4 * 2 * 129
    for bad in ((-1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 129),
                (2 ** 40, 2 ** 20, 2 ** 10, 1, 8)):
        assert workspace(*bad) == -1, bad
    assert isinstance(workspace(1, 1, 1, 1, 1), int) and workspace.restype is ctypes.c_int64


# ------------------------------------------------------------------------------------------------------- the modules
def test_constructor_errors_are_the_references(cusrl):
    for cls in (cusrl.MultiheadAttention, cusrl.MultiheadCrossAttention, cusrl.MultiheadSelfAttention):
        with pytest.raises(ValueError) as raised:
            cls(10, 3)
        assert str(raised.value) == "'embed_dim' (10) must be divisible by 'num_heads' (3)"
    with pytest.raises(ValueError) as raised:
        cusrl.make_norm("batch", 4)
    assert str(raised.value) == "Unsupported normalization type: 'batch'"
    with pytest.raises(ValueError) as raised:
        cusrl.RotaryEmbedding(5)
    assert str(raised.value) == "'head_dim' must be even to use rotary embeddings"
    with pytest.raises(ValueError) as raised:
        cusrl.RotaryEmbedding(4)(torch.zeros(1, 2, 1, 4), offset=-1)
    assert str(raised.value) == "'offset' must be non-negative"
    with pytest.raises(ValueError, match="Unsupported gate type 'lstm'"):
        cusrl.TransformerEncoderLayer(8, 2, gate_type="lstm")
    norm = cusrl.make_norm("rms", 4)
    assert isinstance(norm, torch.nn.RMSNorm) and norm.eps == 1e-6
    norm = cusrl.make_norm("layer", 4)
    assert isinstance(norm, torch.nn.LayerNorm) and norm.eps == 1e-6 and isinstance(cusrl.make_norm(None, 4), torch.nn.Identity)


def test_rotary_cache(cusrl):
    rope = cusrl.RotaryEmbedding(6, max_seq_len=4, base=100.0)
    assert rope.state_dict() == {}, "the buffers are not persistent"
    assert [name for name, _ in rope.named_buffers()] == ["inv_freq", "cos_cached", "sin_cached"]
    assert rope.cos_cached.shape == (4, 3) and (rope.head_dim, rope.max_seq_len, rope.base) == (6, 4, 100.0)
    assert torch.equal(rope.inv_freq, 1.0 / (100.0 ** (torch.arange(0, 6, 2, dtype=torch.float32) / 6)))
    x = torch.randn(2, 5, 3, 6)
    shifted = rope(x, offset=3)
    assert rope.cos_cached.shape == (8, 3), "the cache grows to offset + L"
    assert torch.equal(shifted[:, :2], rope(x[:, :2], offset=3)) and torch.equal(rope(x)[:, 3:], rope(x[:, 3:], offset=3))
    assert not torch.equal(shifted, rope(x)) and torch.equal(rope(x)[:, 0], x[:, 0]), "position 0 is the identity"
    qkv = torch.randn(2, 5, 3, 2, 6)
    rotated = rope.apply_qkv(qkv, offset=1)
    assert rotated.shape == qkv.shape and torch.equal(rotated[:, :, 2], qkv[:, :, 2])
    assert torch.equal(rotated[:, :, 0], rope(qkv[:, :, 0], offset=1)) and torch.equal(rotated[:, :, 1], rope(qkv[:, :, 1], offset=1))


@pytest.mark.parametrize("name", list(_attention.MODULE_CASES))
def test_state_dict_is_the_references(cusrl, golden, name):
    g = golden("attention")
    torch.manual_seed(0)
    module = _attention.build_module(cusrl.nn, name)
    recorded = _attention.recorded_state(g, name + "/")
    assert list(module.state_dict()) == list(recorded)
    for key, value in module.state_dict().items():
        assert value.shape == recorded[key].shape and value.dtype == recorded[key].dtype, key
        if key.endswith(("qkv_proj.bias", "q_proj.bias", "k_proj.bias", "v_proj.bias", "kv_proj.bias")):
            assert not value.any(), f"{key}: the projections' biases start at zero"
    result = module.load_state_dict(recorded, strict=True)
    assert not result.missing_keys and not result.unexpected_keys


@pytest.mark.parametrize("name", list(_attention.MODULE_CASES))
def test_module_reproduces_the_reference(cusrl, golden, name):
    g = golden("attention")
    module = _attention.build_module(cusrl.nn, name)
    module.load_state_dict(_attention.recorded_state(g, name + "/"), strict=True)
    inputs, arguments, w = _attention.recorded_call(g, name)
    before = _launches()
    got = _attention.run_module(module, inputs, arguments, w)
    assert _launches() == before, "a CPU tensor launches nothing"
    _attention.assert_module_matches(name, got, g, name)


def test_the_recorded_masked_row_is_zero_in_the_reference(golden):
    """What the kernels' masked-row rule restates: the reference's CPU run gives a zero attention row there."""
    g = golden("attention")
    _, arguments, _ = _attention.recorded_call(g, "self/8x2/bool")
    assert not arguments["attn_mask"][2].any() and arguments["attn_mask"][[0, 1, 3, 4]].any(-1).all()
    case = _attention.kernel_case(g, (1, 1, 5, 5, 2), "bool", masked_rows=(2,))
    want = _attention.sdpa_formulas(case)
    torch_out = torch.nn.functional.scaled_dot_product_attention(*(case[n].double().transpose(1, 2) for n in ("q", "k", "v")),
                                                                 attn_mask=case["mask"]).transpose(1, 2)
    assert not want["out"][:, 2].any() and not torch_out[:, 2].any() and torch.isinf(want["lse"][..., 2]).all()
    assert torch.allclose(torch_out, want["out"], rtol=1e-6, atol=1e-7)  # (the formulas take the fp32 scale the launch passes)


# ------------------------------------------------------------------------------------------------------------ the ops
def test_cpu_tensors_take_torchs_expression(cusrl, golden):
    from cusrl_amd import ops

    g = golden("attention")
    before = _launches()
    for mask in (None, "causal", "bool", "float"):
        case = _attention.kernel_case(g, (2, 3, 5, 7, 6), mask)
        assert not ops.sdpa_supported(case["q"], case["k"], case["v"], case["mask"], 0.0, case["is_causal"])
        out = ops.sdpa(case["q"], case["k"], case["v"], attn_mask=case["mask"], is_causal=case["is_causal"])
        assert out.shape == case["q"].shape and _attention.relative_to_largest(out, _attention.sdpa_formulas(case)["out"]) <= _attention.BOUND
    rope = cusrl.RotaryEmbedding(6)
    x, dout = _attention.cut(g, "q", (2, 5, 3, 6)), _attention.cut(g, "dout", (2, 5, 3, 6))
    cos, sin = rope._get_cos_sin(5, offset=2)
    assert not ops.rope_supported(x, cos, sin)
    leaf = x.clone().requires_grad_(True)
    out = ops.rope(leaf, cos, sin)
    (dx,) = torch.autograd.grad(out, leaf, dout)
    want = _attention.rope_formulas(x, cos, sin, dout)
    assert _attention.relative_to_largest(out, want["out"]) <= _attention.BOUND and _attention.relative_to_largest(dx, want["dx"]) <= _attention.BOUND
    assert _launches() == before


def test_mask_and_causal_together_are_torchs_business(cusrl):
    """The call is not the kernels' (``sdpa_supported`` refuses it): whatever torch does with it — its error, or its result — is
    what ``ops.sdpa`` and the modules do."""
    from cusrl_amd import ops

    torch.manual_seed(3)
    q, mask = torch.randn(1, 3, 2, 4), torch.ones(3, 3, dtype=torch.bool)
    assert not ops.sdpa_supported(q, q, q, mask, 0.0, True)
    t = q.transpose(1, 2)
    try:
        want = torch.nn.functional.scaled_dot_product_attention(t, t, t, attn_mask=mask, is_causal=True).transpose(1, 2)
    except RuntimeError as torchs:
        with pytest.raises(RuntimeError) as ours:
            ops.sdpa(q, q, q, attn_mask=mask, is_causal=True)
        assert str(ours.value) == str(torchs)
        with pytest.raises(RuntimeError):
            cusrl.MultiheadSelfAttention(8, 2)(torch.zeros(1, 3, 8), attn_mask=mask, is_causal=True)
    else:
        assert torch.equal(ops.sdpa(q, q, q, attn_mask=mask, is_causal=True), want)


class _Device(torch.Tensor):
    """A CPU tensor that says it lives on the device: what ``sdpa_supported`` reads of a tensor, without a GPU."""

    @property
    def is_cuda(self):
        return True


def _device(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Device)


def test_sdpa_supported_refusals(cusrl, monkeypatch):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    N, L, H, D = 2, 5, 3, 4
    q, k, v = _device(N, L, H, D), _device(N, 7, H, D), _device(N, 7, H, D)
    assert ops.sdpa_supported(q, k, v), "the stand-in is accepted: every refusal below is the named one"
    assert ops.sdpa_supported(q, k, v, None, 0.0, True) and ops.sdpa_supported(q, k, v, torch.ones(L, 7, dtype=torch.bool).as_subclass(_Device))
    assert not ops.sdpa_supported(torch.zeros(N, L, H, D), k, v), "a CPU tensor"
    assert not ops.sdpa_supported(_device(N, L, H, D, dtype=torch.float64), k.double(), v.double()), "float64"
    assert not ops.sdpa_supported(q, k.double().as_subclass(_Device), v), "mixed dtypes"
    assert not ops.sdpa_supported(_device(N, L, H, 2 * D)[..., ::2], k, v), "a last-dimension stride of 2"
    assert not ops.sdpa_supported(_device(N, L, D, H).transpose(-1, -2), k, v), "an h stride other than D"
    assert not ops.sdpa_supported(_device(N, L, H, 130), _device(N, 7, H, 130), _device(N, 7, H, 130)), "D beyond the kernel's"
    assert not ops.sdpa_supported(q, k, v, None, 0.1, False), "dropout"
    mask = torch.ones(L, 7, dtype=torch.bool).as_subclass(_Device)
    assert not ops.sdpa_supported(q, k, v, mask, 0.0, True), "a mask and is_causal together"
    assert not ops.sdpa_supported(q, k, v, torch.ones(L, 7, dtype=torch.int32).as_subclass(_Device)), "an integer mask"
    assert not ops.sdpa_supported(q, k, v, torch.ones(L, 7, dtype=torch.float64).as_subclass(_Device)), "a float64 mask"
    assert not ops.sdpa_supported(q, k, v, torch.ones(L, 7).as_subclass(_Device).requires_grad_(True)), "a mask that requires grad"
    assert not ops.sdpa_supported(q, k, v, torch.ones(L, 6, dtype=torch.bool).as_subclass(_Device)), "a mask that does not broadcast"
    assert not ops.sdpa_supported(q, k, v, torch.ones(N, L, 7, dtype=torch.bool).as_subclass(_Device)), "(N, Lq, Lk) broadcasts against H"
    assert not ops.sdpa_supported(q, k, _device(N, 7, H, D + 1)), "values of another width"
    assert not ops.sdpa_supported(q, _device(N, 7, 1, D), _device(N, 7, 1, D)), "fewer key heads"
    # leading dimensions: folded where that is a view and no mask is given
    assert ops.sdpa_supported(_device(L, H, D), _device(7, H, D), _device(7, H, D))
    assert ops.sdpa_supported(_device(2, 3, L, H, D), _device(2, 3, 7, H, D), _device(2, 3, 7, H, D))
    assert not ops.sdpa_supported(_device(3, 2, L, H, D).transpose(0, 1), _device(2, 3, 7, H, D), _device(2, 3, 7, H, D)), "a fold that copies"
    assert not ops.sdpa_supported(_device(L, H, D), _device(7, H, D), _device(7, H, D), mask), "a mask without a batch dimension"
    with monkeypatch.context() as patched:  # (autocast cannot be switched on without a device)
        patched.setattr(torch, "is_autocast_enabled", lambda *device: True)
        assert not ops.sdpa_supported(q, k, v), "autocast"
    leaf = _device(N, L, H, D).requires_grad_(True)
    assert ops.sdpa_supported(leaf, k, v)
    with double_differentiable():
        assert not ops.sdpa_supported(leaf, k, v), "a differentiated forward inside double_differentiable()"
        assert ops.sdpa_supported(q, k, v)
        with torch.no_grad():
            assert ops.sdpa_supported(leaf, k, v)


# ------------------------------------------------------------------------------------------ the algorithm in float32
@pytest.mark.parametrize("shape", _attention.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mask", [None, "causal"])
def test_float32_restatement_meets_the_gpu_bounds(golden, shape, mask):
    """The assertions of tests/test_attention_gpu.py on its shape list, with the tiled online softmax in CPU float32 in the
    kernel's place."""
    case = _attention.kernel_case(golden("attention"), shape, mask)
    want = _attention.sdpa_formulas(case)
    got = _attention.sdpa_restatement(case)
    _attention.assert_sdpa_matches(f"float32 {shape} {mask}", got, want, case)
    assert _attention.relative_to_largest(got["lse"], want["lse"]) <= _attention.BOUND


@pytest.mark.parametrize("mask", ["bool", "float"])
def test_float32_restatement_of_fully_masked_rows(golden, mask):
    rows = (0, 16, 31, 32, 64)  # the first, a middle and the last row, and both sides of the tile edges
    case = _attention.kernel_case(golden("attention"), (2, 2, 65, 70, 8), mask, masked_rows=rows)
    want, got = _attention.sdpa_formulas(case), _attention.sdpa_restatement(case)
    _attention.assert_sdpa_matches(f"float32 masked rows {mask}", got, want, case)
    for result in (want, got):
        assert not result["out"][:, list(rows)].any() and not result["dq"][:, list(rows)].any()
        assert torch.isinf(result["lse"][..., list(rows)]).all() and torch.isfinite(result["lse"][..., 1]).all()


def test_the_formulas_are_the_gradients_of_torchs_attention(golden):
    g = golden("attention")
    for mask in (None, "causal", "bool", "float"):
        case = _attention.kernel_case(g, (2, 3, 5, 7, 6), mask)
        leaves = [case[name].double().requires_grad_(True) for name in ("q", "k", "v")]
        out = torch.nn.functional.scaled_dot_product_attention(*(t.transpose(1, 2) for t in leaves), attn_mask=case["mask"] if mask != "float"
                                                               else case["mask"].double(), is_causal=case["is_causal"]).transpose(1, 2)
        grads = torch.autograd.grad(out, leaves, case["dout"].double())
        want = _attention.sdpa_formulas(case)
        # (the scale is the fp32 1 / sqrt(D) the launch passes: 1e-7 away from torch's float64 one)
        for name, tensor in zip(("out", "dq", "dk", "dv"), (out, *grads)):
            assert _attention.relative_to_largest(want[name], tensor.detach()) <= 5e-7, (mask, name)
        assert math.isclose(float(want["lse"][0, 0, 0]), float(torch.logsumexp(_attention._scores(case, torch.float64)[0][0, 0, 0], -1)))
