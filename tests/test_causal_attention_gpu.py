"""The band attention kernels and the recurrent transformer modules on an MI355X: both entries through ``ops.BandSdpa`` against
the float64 formulas on every shape and option, rows without a visible key, memory safety, reproducibility, packed views, the
dense kernel fed the equivalent mask, the reference's recorded runs (golden ``causal_attention.npz``), the launch budget, and an
agent whose actor runs a ``CausalTransformerEncoderLayer``.

Worst figures measured on an MI355X over every kernel case (what DESIGN.md "Causal sliding-window attention" quotes), relative
to the float64 tensor's largest entry: ``out`` 6.4e-7, ``lse`` 2.3e-7, ``dq`` 8.1e-7, ``dk`` 8.4e-7, ``dv`` 5.3e-7; modules against
the recorded runs at most 1.1e-6."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import _causal_attention as _ca

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD, ROPE, LN_FWD, LN_BWD = ("cusrl_band_sdpa_fwd", "cusrl_band_sdpa_bwd", "cusrl_rope_apply", "cusrl_add_layer_norm_fwd",
                                  "cusrl_add_layer_norm_bwd")
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


def _record(errors: dict):
    for name, error in errors.items():
        WORST[name] = max(WORST.get(name, 0.0), error)


def _sides(case):
    return tuple(None if case[name] is None else case[name].to(DEV) for name in ("key_valid", "q_segment", "alibi_slopes"))


def _band(case, views=None) -> dict:
    """``out``, ``dq``, ``dk``, ``dv`` (from ``key_grad_from`` on) through ``ops.BandSdpa``: one forward launch, one backward call."""
    from cusrl_amd import ops

    q, k, v = views or (case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v"))
    sides, start = _sides(case), case["key_grad_from"]
    assert ops.band_sdpa_supported(q, k, v, case["window"], *sides, start)
    before = _counts()
    out = ops.band_sdpa(q, k, v, case["window"], *sides, key_grad_from=start)
    assert _delta(before)[:2] == (1, 0) and out.is_contiguous()
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case["dout"].to(DEV))
    assert _delta(before)[:2] == (1, 1)
    assert dk.shape == k.shape and not dk[:, :start].any() and not dv[:, :start].any(), "zeros in front of key_grad_from"
    return {"out": out.detach(), "dq": dq, "dk": dk[:, start:], "dv": dv[:, start:]}


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.fixture(scope="module")
def formulas(golden):
    """The float64 expectation of a kernel case, evaluated once per (shape, option) and sliced for ``key_grad_from``."""
    cache = {}

    def get(shape, option, key_grad_from):
        if (shape, option) not in cache:
            cache[shape, option] = _ca.band_formulas(_ca.kernel_case(golden("attention"), shape, option, 0))
        want = cache[shape, option]
        return dict(want, dk=want["dk"][:, key_grad_from:], dv=want["dv"][:, key_grad_from:])

    return get


@pytest.mark.parametrize("shape", _ca.KERNEL_SHAPES + _ca.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("option", _ca.OPTIONS)
def test_kernels_match_the_float64_formulas(cusrl, golden, formulas, shape, option):
    from cusrl_amd.ops.band_attention import _launch_band_fwd

    for key_grad_from in (0, shape[3]):
        case = _ca.kernel_case(golden("attention"), shape, option, key_grad_from)
        want = formulas(shape, option, key_grad_from)
        got = _band(case)
        _record(_ca.assert_sdpa_matches(f"band {shape} {option} from {key_grad_from}", got, want, case))
    _, lse = _launch_band_fwd(*(case[n].to(DEV) for n in ("q", "k", "v")), case["window"], *_sides(case))
    alive = torch.isfinite(want["lse"])
    assert torch.equal(torch.isfinite(lse).cpu(), alive) and (lse.cpu()[~alive] == -math.inf).all()
    if alive.any():
        error = _ca.relative_to_largest(lse.cpu()[alive], want["lse"][alive])
        _record({"lse": error})
        assert error <= _ca.BOUND


@pytest.mark.parametrize("shape", [(2, 2, 35, 20, 8), (2, 2, 35, 20, 6), (3, 2, 1, 20, 8)], ids=lambda s: "x".join(map(str, s)))
def test_a_query_without_a_visible_key(cusrl, golden, shape):
    """Rows made fully invisible through ``key_valid`` (sequence 1: every key): zeros, ``-inf`` and exactly zero gradient
    contributions — the gradients are the bits of the same call with those rows' ``dout`` zeroed."""
    from cusrl_amd.ops.band_attention import _launch_band_fwd

    case = _ca.kernel_case(golden("attention"), shape, "all")
    case["key_valid"][1] = False
    W = shape[3]
    if shape[2] > 1:  # sequence 0: queries 16 and 17 lose every key of their windows, others keep some
        case["key_valid"][0, 16:18 + W] = False
        case["q_segment"][0] = 0
    want, got = _ca.band_formulas(case), _band(case)
    dead = torch.isinf(want["lse"]).all(1)  # [N, Lq]
    assert dead[1].all() and (shape[2] == 1 or (dead[0, 16:18].all() and not dead[0, :16].all()))
    _record(_ca.assert_sdpa_matches(f"band dead rows {shape}", got, want, case))
    _, lse = _launch_band_fwd(*(case[n].to(DEV) for n in ("q", "k", "v")), W, *_sides(case))
    assert not got["out"].cpu()[dead].any() and not got["dq"].cpu()[dead].any() and (lse.cpu().transpose(1, 2)[dead] == -math.inf).all()
    without = dict(case, dout=case["dout"].clone())
    without["dout"][dead] = 0
    again = _band(without)
    assert torch.equal(again["dk"], got["dk"]) and torch.equal(again["dv"], got["dv"]) and torch.equal(again["dq"], got["dq"])


def test_the_dense_kernel_fed_the_equivalent_mask_agrees(cusrl, golden):
    from cusrl_amd import ops

    for shape, option in (((2, 2, 17, 33, 8), "all"), ((2, 3, 5, 7, 6), "valid"), ((1, 2, 40, 31, 4), "segments"), ((3, 2, 1, 17, 8), "all")):
        case = _ca.kernel_case(golden("attention"), shape, option)
        band = _band(case)
        leaves = [case[name].to(DEV).requires_grad_(True) for name in ("q", "k", "v")]
        mask = _ca.dense_equivalent(case).to(DEV)
        assert ops.sdpa_supported(*leaves, mask)
        out = ops.sdpa(*leaves, attn_mask=mask)
        dense = dict(zip(("dq", "dk", "dv"), torch.autograd.grad(out, leaves, case["dout"].to(DEV))), out=out.detach())
        for name in ("out", "dq", "dk", "dv"):
            error = _ca.relative_to_largest(band[name], dense[name])
            assert error <= 2 * _ca.BOUND, f"{shape} {option} {name}: {error:.3e}"


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


@pytest.mark.parametrize("shape,key_grad_from", [((2, 3, 33, 20, 6), 0), ((2, 3, 33, 20, 8), 20), ((1, 2, 17, 16, 128), 7),
                                                 ((3, 2, 1, 17, 8), 0), ((3, 2, 1, 17, 6), 17), ((1, 1, 1, 1, 1), 1)])
def test_launches_stay_inside_their_operands(cusrl, golden, shape, key_grad_from):
    """Guard floats on both sides of every operand untouched, inputs unchanged, NaN-filled outputs fully written, on the 4-byte
    (D = 6, 1) and the 16-byte (D = 8, 128) path, general and step kernel — and the bits of the autograd path."""
    from cusrl_amd import _native

    lib = _native.lib()
    case = _ca.kernel_case(golden("attention"), shape, "all", key_grad_from)
    N, H, Lq, W, D = shape
    Lk, stream = Lq + W, torch.cuda.current_stream().cuda_stream
    ins = {name: _Guarded(case[name].shape, case[name].to(DEV)) for name in ("q", "k", "v", "dout")}
    outs = {"out": _Guarded((N, Lq, H, D)), "lse": _Guarded((N, H, Lq)), "dq": _Guarded((N, Lq, H, D)),
            "dk": _Guarded((N, Lk - key_grad_from, H, D)), "dv": _Guarded((N, Lk - key_grad_from, H, D)),
            "workspace": _Guarded((int(lib.cusrl_band_sdpa_bwd_workspace(N, H, Lq, W, D)),))}
    sides = _sides(case)
    operands = (ins["q"].ptr(), Lq * H * D, H * D, ins["k"].ptr(), Lk * H * D, H * D, ins["v"].ptr(), Lk * H * D, H * D,
                *(side.data_ptr() for side in sides), 1.0 / math.sqrt(D), outs["out"].ptr(), outs["lse"].ptr())
    fwd = lib.cusrl_band_sdpa_fwd(*operands, N, H, Lq, W, D, stream)
    bwd = lib.cusrl_band_sdpa_bwd(*operands, ins["dout"].ptr(), Lq * H * D, H * D, key_grad_from, outs["dq"].ptr(), outs["dk"].ptr(),
                                  outs["dv"].ptr(), outs["workspace"].ptr(), N, H, Lq, W, D, stream)
    torch.cuda.synchronize()
    assert (fwd, bwd) == (0, 0)
    for name, guarded in {**ins, **outs}.items():
        assert guarded.guards_intact(), name
        assert not torch.isnan(guarded.tensor).any(), f"{name}: not fully written"
    for name, guarded in ins.items():
        assert torch.equal(guarded.tensor, guarded.before), name
    expected = _band(case)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(outs[name].tensor, expected[name]), name


@pytest.mark.parametrize("shape", [(2, 2, 33, 17, 24), (1, 2, 40, 31, 4), (1, 2, 40, 32, 3)], ids=lambda s: "x".join(map(str, s)))
def test_the_backward_gives_the_same_bits_every_time(cusrl, golden, shape):
    case = _ca.kernel_case(golden("attention"), shape, "all")
    first, second = _band(case), _band(case)
    assert all(torch.equal(first[name], second[name]) for name in first)


@pytest.mark.parametrize("shape", [(2, 2, 17, 33, 8), (1, 2, 40, 31, 4), (2, 3, 33, 20, 6)], ids=lambda s: "x".join(map(str, s)))
def test_key_grad_from_gives_the_rows_of_the_whole_backward(cusrl, golden, shape):
    """The key-major pass started at key 7 or at key ``W`` stores the bits of rows ``key_grad_from:`` of the pass started at key
    0, and ``dq`` does not move: wherever an owner's query tiles start it adds its terms in query order, and a query outside the
    band contributes a product with an exact zero."""
    from cusrl_amd.ops.band_attention import _launch_band_fwd, band_sdpa_backward

    case = _ca.kernel_case(golden("attention"), shape, "all")
    q, k, v, dout = (case[name].to(DEV) for name in ("q", "k", "v", "dout"))
    window, sides = shape[3], _sides(case)
    out, lse = _launch_band_fwd(q, k, v, window, *sides)
    dq, dk, dv = band_sdpa_backward(q, k, v, out, lse, dout, window, *sides)
    for start in (7, window):
        dq_from, dk_from, dv_from = band_sdpa_backward(q, k, v, out, lse, dout, window, *sides, key_grad_from=start)
        assert torch.equal(dq_from, dq), start
        assert torch.equal(dk_from, dk[:, start:]) and torch.equal(dv_from, dv[:, start:]), start


@pytest.mark.parametrize("D", [8, 6])
def test_packed_kv_views_launch_where_they_are(cusrl, golden, monkeypatch, D):
    """The two slices of a packed ``[N, Lk, 2, H, D]`` projection are what the launch sees (their own data pointers and strides)
    and give the bits of their contiguous copies; so does a ``[L, N, H, D]`` query transposed."""
    from cusrl_amd.ops import band_attention

    N, H, L, W = 2, 3, 19, 5
    case = _ca.kernel_case(golden("attention"), (N, H, L, W, D), "all", W)
    seen = []
    real_fwd, real_bwd = band_attention._checked.cusrl_band_sdpa_fwd, band_attention._checked.cusrl_band_sdpa_bwd
    monkeypatch.setattr(band_attention._checked, "cusrl_band_sdpa_fwd", lambda *a: (seen.append(a[:9]), real_fwd(*a))[1])
    monkeypatch.setattr(band_attention._checked, "cusrl_band_sdpa_bwd", lambda *a: (seen.append(a[:9]), real_bwd(*a))[1])
    plain = _band(case)
    seen.clear()
    kv = torch.stack([case["k"], case["v"]], dim=2).to(DEV).requires_grad_(True)
    k, v = kv.unbind(dim=2)
    q = case["q"].to(DEV).transpose(0, 1).contiguous().requires_grad_(True)  # [L, N, H, D]
    packed = _band(case, (q.transpose(0, 1), k, v))
    row = 2 * H * D
    assert len(seen) == 2 and v.data_ptr() - k.data_ptr() == 4 * H * D
    for a in seen:
        assert a == (q.data_ptr(), H * D, N * H * D, k.data_ptr(), (L + W) * row, row, v.data_ptr(), (L + W) * row, row)
    assert all(torch.equal(packed[name], plain[name]) for name in plain)


def test_error_codes_on_the_device_write_nothing(cusrl):
    from cusrl_amd import _native

    lib, invalid = _native.lib(), _native._CONSTANTS["E_INVALID"]
    stream = torch.cuda.current_stream().cuda_stream
    out, lse = _Guarded((2, 3, 2, 4)), _Guarded((2, 2, 3))
    p = torch.zeros(2, 5, 2, 4, device=DEV).data_ptr()
    common = (p, 24, 8, p, 40, 8, p, 40, 8, None, None, None, 0.5)
    assert lib.cusrl_band_sdpa_fwd(*common, out.ptr(), lse.ptr(), 2, 2, 3, 0, 4, stream) == invalid
    assert lib.cusrl_band_sdpa_fwd(*common, out.ptr(), lse.ptr(), 2, 2, 3, 2, 129, stream) == invalid
    assert lib.cusrl_band_sdpa_fwd(*common, out.ptr(), None, 2, 2, 3, 2, 4, stream) == invalid
    assert lib.cusrl_band_sdpa_fwd(*common, out.ptr(), lse.ptr(), 0, 2, 3, 2, 4, stream) == 0
    assert lib.cusrl_band_sdpa_bwd(*common, p, p, p, 24, 8, 3, out.ptr(), out.ptr(), out.ptr(), lse.ptr(), 2, 2, 3, 2, 4, stream) == invalid
    assert lib.cusrl_band_sdpa_bwd(*common, p, p, p, 24, 8, 0, out.ptr(), out.ptr(), out.ptr(), None, 2, 2, 3, 2, 4, stream) == invalid
    torch.cuda.synchronize()
    assert torch.isnan(out.tensor).all() and torch.isnan(lse.tensor).all() and out.guards_intact() and lse.guards_intact()


# ------------------------------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("name", list(_ca.MODULE_CASES))
def test_module_reproduces_the_reference_on_the_device(cusrl, golden, name):
    g = golden("causal_attention")
    module = _ca.build_module(cusrl.nn, name, cusrl.get_alibi_slopes).to(DEV)
    module.load_state_dict(_ca._attention.recorded_state(g, name + "/"), strict=True)
    before = _counts()
    got = _ca.run_case(module, name, _ca.recorded_inputs(g, name), torch.from_numpy(g[name + "/w"].copy()), device=DEV)
    fwd, bwd = _delta(before)[:2]
    assert (fwd, bwd) == (1 + ("warmup" in _ca.recorded_inputs(g, name)), 1), "the band kernels carried it"
    _record({"modules": _ca.assert_case_matches(name, {key: value.cpu() for key, value in got.items()}, g, name, cache_exact=False)})


def test_launch_budget(cusrl):
    torch.manual_seed(5)
    x = torch.randn(7, 3, 8, device=DEV)
    done = torch.zeros(7, 3, 1, dtype=torch.bool, device=DEV)
    done[2, 1] = True
    for rope_base, ropes in ((None, 0), (100.0, 2)):
        module = cusrl.CausalMultiheadSelfAttention(8, 2, 4, rope_base=rope_base, alibi_slopes=[0.5, 0.25]).to(DEV)
        before = _counts()
        out, memory = module(x.clone().requires_grad_(True), None, done=done)
        assert _delta(before)[:3] == (1, 0, ropes)
        out.sum().backward()
        assert _delta(before)[:3] == (1, 1, 2 * ropes)
        before = _counts()
        with torch.no_grad():
            module(x[0], memory)
        assert _delta(before)[:3] == (1, 0, ropes), "a step without a gradient: the forward launch alone"
    for kwargs in (dict(), dict(layer_norm="pre")):
        layer = cusrl.CausalTransformerEncoderLayer(8, 2, 4, **kwargs).to(DEV)
        before = _counts()
        out, _ = layer(x.clone().requires_grad_(True), None, done=done)
        assert _delta(before) == (1, 0, 0, 2, 0)
        out.sum().backward()
        assert _delta(before) == (1, 1, 0, 2, 2)


def test_fallbacks_launch_nothing(cusrl, golden):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    case = _ca.kernel_case(golden("attention"), (2, 3, 5, 7, 6), "slopes")
    q, k, v = (case[n].to(DEV) for n in ("q", "k", "v"))
    slopes = case["alibi_slopes"].to(DEV)
    want = _ca.band_formulas(case)["out"]
    before = _counts()
    assert _ca.relative_to_largest(ops.band_sdpa(q.double(), k.double(), v.double(), 7, alibi_slopes=slopes), want) <= 1e-6
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not ops.band_sdpa_supported(q, k, v, 7)
    leaf = q.clone().requires_grad_(True)
    with double_differentiable():
        out = ops.band_sdpa(leaf, k, v, 7, alibi_slopes=slopes)
        (grad,) = torch.autograd.grad(out.sum(), leaf, create_graph=True)
        assert grad.requires_grad or not grad.any()
    assert _delta(before)[:2] == (0, 0)
    module = cusrl.CausalMultiheadSelfAttention(8, 2, 4, dtype=torch.bfloat16).to(DEV)
    out, memory = module(torch.randn(5, 2, 8, device=DEV))
    assert out.dtype == torch.float32 and torch.isfinite(out).all() and memory["cache_mask"].all() and _delta(before)[:2] == (0, 0)


# ------------------------------------------------------------------------------------------------------------ an agent
def test_agent_with_a_causal_transformer_backbone_trains(cusrl):
    """The actor's backbone is a ``CausalTransformerEncoderLayer`` in the eager ``ppo`` preset: 8 envs, 8 steps per update, 2 epochs
    x 2 minibatches, 3 iterations.  Its dict memory makes the sampler temporal; the band entries carry every ``act()`` and every
    minibatch step."""
    cusrl.set_global_seed(17)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=12, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2).to_underlying()
    factory.actor_factory.backbone_factory = cusrl.CausalTransformerEncoderLayer.Factory(embed_dim=16, num_heads=2, window_size=4,
                                                                                         rope_base=100.0)
    trainer = cusrl.Trainer(env, factory, num_iterations=3, verbose=False)
    agent = trainer.agent
    assert isinstance(agent.actor.backbone, cusrl.CausalTransformerEncoderLayer) and agent.actor.is_recurrent
    initial = {name: param.detach().clone() for name, param in agent.named_parameters()}
    start = _counts()
    trainer.run_training_loop()
    torch.cuda.synchronize()
    fwd, bwd, rope, ln_fwd, ln_bwd = _delta(start)
    print(f"launches: band fwd {fwd} bwd {bwd}, rope {rope}, add_layer_norm fwd {ln_fwd} bwd {ln_bwd}")
    assert fwd >= 3 * (8 + 2 * 2) and bwd >= 3 * 2 * 2 and rope >= 2 * fwd + 2 * bwd and ln_fwd >= 2 * fwd and ln_bwd >= 2 * bwd
    storage = list(agent.buffer.storage)
    assert any(key.startswith("actor_memory") and "input_cache" in key for key in storage), storage
    assert any(key.startswith("actor_memory") and "cache_mask" in key for key in storage), storage
    assert isinstance(agent.actor_memory, dict) and agent.actor_memory["cache_mask"].dtype == torch.bool
    assert np.isfinite(trainer.last_info["Agent/value_loss"])
    for name, param in agent.named_parameters():
        assert torch.isfinite(param).all(), name
        if param.requires_grad:
            assert not torch.equal(param, initial[name]), f"{name} did not change"


def test_worst_measured_errors_are_printed():
    print("worst measured, relative to the largest entry: " + ", ".join(f"{name} {error:.3e}" for name, error in sorted(WORST.items())))
    assert WORST and max(WORST.values()) <= _ca.BOUND
