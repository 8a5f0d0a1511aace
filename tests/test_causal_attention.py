"""Causal sliding-window attention without a GPU: the public surface, the reference's recorded state dicts and runs (golden
``causal_attention.npz``) through the dense-mask fallback, the memory's consistency between a whole sequence and its steps, what
``band_sdpa_supported`` refuses, and the raw entries' argument validation."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import _causal_attention as _ca

NAMES = ["CausalMultiheadSelfAttention", "CausalTransformerEncoderLayer", "compute_segment_ids", "get_alibi_slopes"]
SYMBOLS = {"cusrl_band_sdpa_fwd", "cusrl_band_sdpa_bwd", "cusrl_band_sdpa_bwd_workspace"}
OPS = ("band_sdpa", "band_sdpa_supported", "band_sdpa_backward", "BandSdpa")


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def _launches():
    from cusrl_amd import _native

    return dict(_native.launch_counts)


def test_names_are_exported_from_every_namespace(cusrl):
    import cusrl_amd.nn.causal_attn
    from cusrl_amd import ops

    assert set(cusrl.nn.causal_attn.__all__) == set(NAMES)
    for namespace in (cusrl, cusrl.nn):
        assert set(NAMES) <= set(namespace.__all__)
        for name in NAMES:
            assert getattr(namespace, name) is getattr(cusrl.nn.causal_attn, name)
    for name in OPS:
        assert hasattr(ops, name), name
    assert cusrl.CausalMultiheadSelfAttention.Factory(8, 2, 4)(input_dim=5).input_dim == 5
    layer = cusrl.CausalTransformerEncoderLayer.Factory(embed_dim=8, num_heads=2, window_size=4, rope_base=100.0)(input_dim=5, output_dim=3)
    assert (layer.input_dim, layer.output_dim, layer.is_recurrent, layer.self_attn.is_recurrent) == (5, 3, True, True)


def test_abi_stays_7_and_the_new_symbols_are_bound():
    from cusrl_amd import _native

    assert _native.ABI_VERSION == 7
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    for symbol in SYMBOLS:
        assert hasattr(_native.lib(), symbol)


def test_raw_entries_refuse_bad_arguments_without_a_gpu():
    """Argument validation runs on the host before anything is launched: every refusal is ``CUSRL_E_INVALID``."""
    from cusrl_amd import _native

    lib, invalid = _native.lib(), _native._CONSTANTS["E_INVALID"]
    a = 4096  # (a non-NULL address nothing dereferences: the entries return before a launch)
    sizes = dict(N=2, H=2, Lq=3, W=2, D=4)

    def fwd(q=a, k=a, v=a, valid=None, segment=None, slopes=None, out=a, lse=a, **changed):
        s = {**sizes, **changed}
        return lib.cusrl_band_sdpa_fwd(q, 24, 8, k, 40, 8, v, 40, 8, valid, segment, slopes, 0.5, out, lse, s["N"], s["H"], s["Lq"], s["W"],
                                       s["D"], None)

    def bwd(q=a, k=a, v=a, valid=None, segment=None, slopes=None, out=a, lse=a, dout=a, key_grad_from=0, dq=a, dk=a, dv=a, workspace=a,
            **changed):
        s = {**sizes, **changed}
        return lib.cusrl_band_sdpa_bwd(q, 24, 8, k, 40, 8, v, 40, 8, valid, segment, slopes, 0.5, out, lse, dout, 24, 8, key_grad_from, dq, dk,
                                       dv, workspace, s["N"], s["H"], s["Lq"], s["W"], s["D"], None)

    for name in ("q", "k", "v", "out", "lse"):
        assert fwd(**{name: None}) == invalid, name
    for name in ("q", "k", "v", "out", "lse", "dout", "dq", "dk", "dv", "workspace"):
        assert bwd(**{name: None}) == invalid, name
    for call in (fwd, bwd):
        for changed in (dict(N=-1), dict(H=0), dict(H=-1), dict(Lq=0), dict(Lq=-3), dict(W=0), dict(W=-1), dict(D=0), dict(D=129), dict(D=-4)):
            assert call(**changed) == invalid, changed
        assert call(N=0) == 0, "N == 0 is a successful no-op"
        assert call(N=0, Lq=1) == 0
    for key_grad_from in (-1, 3):
        assert bwd(key_grad_from=key_grad_from) == invalid, key_grad_from
    assert bwd(N=0, key_grad_from=2) == 0 and bwd(N=0, workspace=None) == 0


def test_workspace_helper():
    from cusrl_amd import _native

    workspace = _native.lib().cusrl_band_sdpa_bwd_workspace
    assert workspace(2, 3, 5, 7, 6) == 2 * 3 * 5, "delta: one float per (n, h, query row)"
    assert workspace(1, 1, 1, 1, 1) == 1 and workspace(0, 2, 5, 7, 6) == 0
    assert workspace(4, 2, 129, 1, 128) == 4 * 2 * 129
    for bad in ((-1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 129),
                (2 ** 40, 2 ** 20, 2 ** 10, 1, 8), (1, 1, 2 ** 62, 2 ** 62, 1)):
        assert workspace(*bad) == -1, bad
    assert isinstance(workspace(1, 1, 1, 1, 1), int) and workspace.restype is ctypes.c_int64


# ------------------------------------------------------------------------------------------------------- the modules
def test_constructor_errors_are_the_references(cusrl):
    attention = cusrl.CausalMultiheadSelfAttention
    for arguments, text in (
        (dict(embed_dim=10, num_heads=3, window_size=4), "'embed_dim' must be divisible by 'num_heads'"),
        (dict(embed_dim=8, num_heads=2, window_size=4, rope_base=0.0), "'rope_base' must be a positive number"),
        (dict(embed_dim=6, num_heads=2, window_size=4, rope_base=100.0), "'head_dim' must be even when RoPE is enabled"),
        (dict(embed_dim=8, num_heads=2, window_size=4, alibi_slopes=torch.ones(2, 1)), "'alibi_slopes' must be a 1D tensor"),
        (dict(embed_dim=8, num_heads=2, window_size=4, alibi_slopes=[0.5, 0.25, 0.125]), "'alibi_slopes' must contain 2 elements"),
        (dict(embed_dim=8, num_heads=2, window_size=0), "'window_size' must be a positive integer"),
    ):
        with pytest.raises(ValueError) as raised:
            attention(**arguments)
        assert str(raised.value) == text
    with pytest.raises(ValueError, match="Unsupported gate type 'lstm'"):
        cusrl.CausalTransformerEncoderLayer(8, 2, 4, gate_type="lstm")
    module = attention(8, 2, 4, alibi_slopes=[0.5, 0.25])
    assert "alibi_slopes" not in module.state_dict() and module.alibi_slopes.dtype == torch.float32, "a non-persistent buffer"
    assert attention(8, 2, 4).alibi_slopes is None and attention(8, 2, 4).rope is None
    layer = cusrl.CausalTransformerEncoderLayer(6, 3, 4, use_alibi=True)
    assert torch.equal(layer.self_attn.alibi_slopes, torch.tensor(cusrl.get_alibi_slopes(3)))


def test_alibi_slopes_and_segment_ids_are_the_references(cusrl, golden):
    g = golden("causal_attention")
    for heads in (1, 2, 3, 4, 6, 8, 12):
        assert np.array_equal(np.array(cusrl.get_alibi_slopes(heads), dtype=np.float64), g[f"alibi_slopes/{heads}"]), heads
    done = torch.from_numpy(g["segments/done"])
    q_segments, kv_segments = cusrl.compute_segment_ids(done, 4)
    assert q_segments.dtype == torch.int32 and kv_segments.dtype == torch.int32
    assert np.array_equal(q_segments.numpy(), g["segments/q"]) and np.array_equal(kv_segments.numpy(), g["segments/kv"])


@pytest.mark.parametrize("name", list(_ca.MODULE_CASES))
def test_state_dict_is_the_references(cusrl, golden, name):
    g = golden("causal_attention")
    torch.manual_seed(0)
    module = _ca.build_module(cusrl.nn, name, cusrl.get_alibi_slopes)
    recorded = _ca._attention.recorded_state(g, name + "/")
    assert list(module.state_dict()) == list(recorded)
    for key, value in module.state_dict().items():
        assert value.shape == recorded[key].shape and value.dtype == recorded[key].dtype, key
    result = module.load_state_dict(recorded, strict=True)
    assert not result.missing_keys and not result.unexpected_keys


@pytest.mark.parametrize("name", list(_ca.MODULE_CASES))
def test_module_reproduces_the_reference(cusrl, golden, name):
    g = golden("causal_attention")
    module = _ca.build_module(cusrl.nn, name, cusrl.get_alibi_slopes)
    module.load_state_dict(_ca._attention.recorded_state(g, name + "/"), strict=True)
    before = _launches()
    got = _ca.run_case(module, name, _ca.recorded_inputs(g, name), torch.from_numpy(g[name + "/w"].copy()))
    assert _launches() == before, "a CPU tensor launches nothing"
    exact = _ca.cache_is_a_copy(name)
    _ca.assert_case_matches(name, got, g, name, cache_exact=exact)
    if not exact:
        # the layer computed what its attention saw (in_proj, the pre-norm): the recorded bits are another machine's GEMM and
        # LayerNorm, so the cache is held bit for bit to that computation made here: its last W rows, batch first
        with torch.no_grad():
            seen = module.in_proj(_ca.recorded_inputs(g, name)["input"])
            seen = module.norm1(seen) if module.layer_norm == "pre" else seen
        assert seen.shape[0] >= _ca.W
        assert torch.equal(got["memory/input_cache"], seen[-_ca.W:].transpose(0, 1).flatten(1))


@pytest.mark.parametrize("kwargs", [dict(), dict(rope_base=100.0), dict(use_alibi=True, rope_base=100.0, layer_norm="pre", gate_type="gru")],
                         ids=["plain", "rope", "alibi_rope_pre_gru"])
def test_sequence_equals_its_steps(cusrl, kwargs):
    """The reference's own consistency test: the whole ``[L, N, C]`` sequence with ``done`` against one step at a time with
    ``reset_memory`` in between.  Each side is within BOUND of the exact result, so they are within 2 BOUND of each other."""
    torch.manual_seed(5)
    L, N, C, W = 11, 3, 8, 4
    layer = cusrl.CausalTransformerEncoderLayer(C, 2, W, feedforward_dim=16, **kwargs)
    x = torch.randn(L, N, C)
    done = torch.zeros(L, N, 1, dtype=torch.bool)
    for step, env in ((0, 0), (4, 1), (5, 1), (10, 2), (7, 0)):
        done[step, env] = True
    with torch.no_grad():
        whole, memory = layer(x, None, done=done)
        steps, step_memory, stepped = [], None, None
        for t in range(L):
            stepped = layer.step_memory(x[t], step_memory)
            output, step_memory = layer(x[t], step_memory)
            assert torch.equal(stepped["input_cache"], step_memory["input_cache"]) and torch.equal(stepped["cache_mask"], step_memory["cache_mask"])
            layer.reset_memory(step_memory, done[t])
            steps.append(output)
    error = _ca.relative_to_largest(torch.stack(steps), whole)
    print(f"sequence against steps: {error:.3e}")
    assert error <= 2 * _ca.BOUND
    layer.reset_memory(memory, done[-1])
    assert torch.equal(memory["cache_mask"], step_memory["cache_mask"])
    assert torch.equal(memory["input_cache"] * memory["cache_mask"].repeat_interleave(C, -1), step_memory["input_cache"] * step_memory["cache_mask"].repeat_interleave(C, -1))
    layer.reset_memory(memory)
    assert not memory["cache_mask"].any() and not memory["input_cache"].any()
    layer.reset_memory(None)


# ------------------------------------------------------------------------------------------------------------ the ops
@pytest.mark.parametrize("option", _ca.OPTIONS)
def test_cpu_tensors_take_the_dense_mask(golden, option):
    """The fallback (a dense mask through ``ops.sdpa``) against the float64 formulas, gradients included."""
    from cusrl_amd import ops

    g = golden("attention")
    before = _launches()
    for shape, key_grad_from in (((2, 3, 5, 7, 6), 0), ((2, 2, 17, 3, 4), 3), ((3, 2, 1, 5, 4), 5)):
        case = _ca.kernel_case(g, shape, option, key_grad_from)
        if case["key_valid"] is not None:  # (torch's softmax has no rule for a row without a key: keep every query's own token)
            case["key_valid"][:, case["window"]:] = True
        sides = (case["key_valid"], case["q_segment"], case["alibi_slopes"])
        leaves = [case[name].clone().requires_grad_(True) for name in ("q", "k", "v")]
        assert not ops.band_sdpa_supported(*leaves, case["window"], *sides)
        out = ops.band_sdpa(*leaves, case["window"], *sides, key_grad_from=key_grad_from)
        dq, dk, dv = torch.autograd.grad(out, leaves, case["dout"])
        assert not dk[:, :key_grad_from].any() and not dv[:, :key_grad_from].any()
        got = {"out": out.detach(), "dq": dq, "dk": dk[:, key_grad_from:], "dv": dv[:, key_grad_from:]}
        _ca.assert_sdpa_matches(f"fallback {shape} {option}", got, _ca.band_formulas(case), case)
        double = ops.band_sdpa(*(t.detach().double() for t in leaves), case["window"], *sides)
        assert double.dtype == torch.float64 and _ca.relative_to_largest(double, _ca.band_formulas(case)["out"]) <= 1e-6
    assert _launches() == before


def test_band_sdpa_refuses_wrong_shapes():
    from cusrl_amd import ops

    q, k = torch.zeros(2, 5, 3, 4), torch.zeros(2, 9, 3, 4)
    ops.band_sdpa(q, k, k, 4)
    for arguments in ((q, k, k, 3), (q, k, k, 0), (q, k, k[:, :8], 4), (q[0], k[0], k[0], 4)):
        with pytest.raises(ValueError):
            ops.band_sdpa(*arguments)
    for sides in (dict(key_valid=torch.ones(2, 8, dtype=torch.bool)), dict(q_segment=torch.zeros(2, 9, dtype=torch.int32)),
                  dict(alibi_slopes=torch.ones(2)), dict(key_grad_from=5), dict(key_grad_from=-1)):
        with pytest.raises(ValueError):
            ops.band_sdpa(q, k, k, 4, **sides)


class _Device(torch.Tensor):
    """A CPU tensor that says it lives on the device: what ``band_sdpa_supported`` reads of a tensor, without a GPU."""

    @property
    def is_cuda(self):
        return True


def _device(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Device)


def test_band_sdpa_supported_refusals(monkeypatch):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    N, L, H, D, W = 2, 5, 3, 4, 2
    q, k, v = _device(N, L, H, D), _device(N, L + W, H, D), _device(N, L + W, H, D)
    valid, segment, slopes = _device(N, L + W, dtype=torch.bool), _device(N, L, dtype=torch.int32), _device(H)
    assert ops.band_sdpa_supported(q, k, v, W), "the stand-in is accepted: every refusal below is the named one"
    assert ops.band_sdpa_supported(q, k, v, W, valid, segment, slopes) and ops.band_sdpa_supported(q, k, v, W, valid.to(torch.uint8).as_subclass(_Device))
    packed = _device(N, L + W, 2, H, D)
    assert ops.band_sdpa_supported(q, *packed.unbind(2), W), "the two slices of a packed projection"
    assert not ops.band_sdpa_supported(torch.zeros(N, L, H, D), k, v, W), "a CPU tensor"
    assert not ops.band_sdpa_supported(_device(N, L, H, D, dtype=torch.float64), k.double(), v.double(), W), "float64"
    assert not ops.band_sdpa_supported(_device(N, L, H, D, dtype=torch.bfloat16), k.bfloat16(), v.bfloat16(), W), "bfloat16"
    assert not ops.band_sdpa_supported(_device(N, L, H, 2 * D)[..., ::2], k, v, W), "a last-dimension stride of 2"
    assert not ops.band_sdpa_supported(_device(N, L, D, H).transpose(-1, -2), k, v, W), "an h stride other than D"
    assert not ops.band_sdpa_supported(_device(N, L, H, 130), _device(N, L + W, H, 130), _device(N, L + W, H, 130), W), "D beyond the kernel's"
    assert not ops.band_sdpa_supported(q, k, v, W, _device(N, L + W, dtype=torch.int32)), "an int32 key_valid"
    assert not ops.band_sdpa_supported(q, k, v, W, None, _device(N, L, dtype=torch.int64)), "int64 segments"
    assert not ops.band_sdpa_supported(q, k, v, W, None, None, _device(H, dtype=torch.float64)), "float64 slopes"
    assert not ops.band_sdpa_supported(q, k, v, W, None, _device(L, N, dtype=torch.int32).t()), "segments that are not contiguous"
    assert not ops.band_sdpa_supported(q, k, v, W, None, None, _device(H).requires_grad_(True)), "slopes that require grad"
    with monkeypatch.context() as patched:  # (autocast cannot be switched on without a device)
        patched.setattr(torch, "is_autocast_enabled", lambda *device: True)
        assert not ops.band_sdpa_supported(q, k, v, W), "autocast"
    leaf = _device(N, L, H, D).requires_grad_(True)
    assert ops.band_sdpa_supported(leaf, k, v, W)
    with double_differentiable():
        assert not ops.band_sdpa_supported(leaf, k, v, W), "a differentiated forward inside double_differentiable()"
        assert ops.band_sdpa_supported(q, k, v, W)
