"""The depthwise-convolution kernels, SeparableConv2d, Cnn and the 2-D positional encodings on an MI355X: the three launches
against the float64 evaluation of their formulas under derived bounds, unread positions, determinism, memory safety, offset and
channels_last operands, the launch census, fallback predicates, the reference's recorded runs (golden ``cnn.npz``) and an agent
whose actor encodes its observation with a ``Cnn``.

No test here calls torch's convolution on the device: every expectation is a float64 CPU evaluation or a recorded run.

Worst figures measured on an MI355X over every kernel case (what DESIGN.md "Depthwise convolution" quotes): ``out`` 0.80 and
``dx`` 0.47 of the bound gamma(K + 1) * sum |terms| (both at the single-tap 1 x 1 case; 0.10 / 0.087 at ``[130, 3, 17, 16]`` k7 p3
and 0.22 / 0.23 at the dilated, strided geometry), ``dw`` 5.5e-8 and ``dbias`` 4.6e-8 of the largest entry; modules against the
recorded runs at most 3.0e-7 of the largest entry."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _cnn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD_INPUT, BWD_PARAMS = _cnn.LAUNCHES
GUARD = 64  # floats on either side of an operand (256 bytes: the operand keeps its 16-byte alignment)
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _counts():
    from cusrl_amd import _native

    return tuple(_native.launch_counts.get(symbol, 0) for symbol in _cnn.LAUNCHES)


def _delta(before):
    return tuple(now - then for now, then in zip(_counts(), before))


def _on_device(case):
    return {key: value.to(DEV) if isinstance(value, torch.Tensor) else value for key, value in case.items()}


def _arguments(case):
    KH, KW, SH, SW, PH, PW, DH, DW = case["geometry"]
    return (SH, SW), (PH, PW), (DH, DW)


def _forward_backward(case) -> dict:
    """``out``, ``dx``, ``dw`` and ``dbias`` through the autograd Function: one forward launch, one launch of each backward."""
    from cusrl_amd import ops

    leaves = [None if case[name] is None else case[name].detach().requires_grad_(True) for name in ("x", "w", "bias")]
    assert ops.dwconv2d_supported(*leaves, *_arguments(case))
    before = _counts()
    out = ops.depthwise_conv2d(*leaves, *_arguments(case))
    assert _delta(before) == (1, 0, 0)
    grads = iter(torch.autograd.grad(out, [leaf for leaf in leaves if leaf is not None], grad_outputs=case["dout"]))
    assert _delta(before) == (1, 1, 1), "one forward launch and one of each backward"
    return {"out": out.detach(), "dx": next(grads), "dw": next(grads), "dbias": None if case["bias"] is None else next(grads)}


def _same(a: dict, b: dict) -> bool:
    return sorted(a) == sorted(b) and all((a[key] is None and b[key] is None) or torch.equal(a[key], b[key]) for key in a)


_WORST: dict[str, float] = {}


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("label,N,C", _cnn.KERNEL_CASES)
def test_kernels_match_the_float64_formulas(cusrl, golden, label, N, C):
    from cusrl_amd import _native

    case = _cnn.kernel_case(golden("cnn"), label, N, C)
    got = _forward_backward(_on_device(case))
    errors = _cnn.assert_kernel_matches(f"{label} [{N}, {C}]", got, case)
    for name, error in errors.items():
        _WORST[name] = max(_WORST.get(name, 0.0), error)
    unread = _cnn.unread_positions(case)
    assert not got["dx"].cpu()[:, :, unread].any(), "a position no window reads has a gradient"
    if label == "8x8 k3 s2":
        assert unread[7].all() and unread[:, 7].all()
    needed = _native.lib().cusrl_dwconv2d_num_partials(*case["dout"].shape)
    if (label, N) == ("17x16 k7 p3", 130):
        assert needed > 1, "the finalize launch is exercised"
    if N <= 3:
        assert needed == 0, "one block per channel writes dw and dbias itself"


def test_worst_measured_errors_are_printed():
    """(runs after the parity cases of this module: what DESIGN.md quotes)"""
    for name, error in sorted(_WORST.items()):
        unit = "of the gamma bound" if name in ("out", "dx") else "of the largest entry"
        print(f"worst over every kernel case, {name}: {error:.3e} {unit}")


def test_parameter_gradients_are_deterministic(cusrl, golden):
    from cusrl_amd import ops

    for label, N, C in (("17x16 k7 p3", 130, 3), ("33x9 k(5,3) s(2,1) p(2,3) d(2,1)", 130, 3), ("5x7 k3", 3, 3)):
        case = _on_device(_cnn.kernel_case(golden("cnn"), label, N, C))
        first = ops.dwconv2d_backward_params(case["x"], case["dout"], case["geometry"])
        second = ops.dwconv2d_backward_params(case["x"], case["dout"], case["geometry"])
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), label
        only_weight = ops.dwconv2d_backward_params(case["x"], case["dout"], case["geometry"], with_bias=False)
        assert only_weight[1] is None and torch.equal(only_weight[0], first[0])


# ------------------------------------------------------------------------------------------------ memory safety, raw entry points
def _raw(name):
    from cusrl_amd import _native

    return getattr(_native.lib(), name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """A tensor inside a buffer with ``GUARD`` sentinel floats on either side; ``values`` None: an output, filled with NaN."""

    def __init__(self, shape, values=None, dtype=torch.float32):
        numel = int(np.prod(shape))
        self.buffer = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.tensor = self.buffer[GUARD:GUARD + numel].view(shape)
        self.tensor.copy_(values) if values is not None else self.tensor.fill_(float("nan"))
        self.before = self.tensor.clone()

    def guards_intact(self) -> bool:
        return bool((self.buffer[:GUARD] == SENTINEL).all() and (self.buffer[-GUARD:] == SENTINEL).all())

    def unchanged(self) -> bool:
        return torch.equal(self.tensor, self.before)

    def ptr(self):
        return self.tensor.data_ptr()


@pytest.mark.parametrize("label,N,C", [("17x16 k7 p3", 130, 3), ("33x9 k(5,3) s(2,1) p(2,3) d(2,1)", 3, 3)])
def test_launches_stay_inside_their_operands(cusrl, golden, label, N, C):
    """Guard floats on both sides of every operand untouched, inputs unchanged, NaN-filled outputs fully written — and the bits
    of the autograd Function's call."""
    from cusrl_amd import _native

    case = _on_device(_cnn.kernel_case(golden("cnn"), label, N, C))
    expected = _forward_backward(case)
    inputs = {name: _Guarded(case[name].shape, case[name]) for name in ("x", "w", "bias", "dout")}
    outputs = {name: _Guarded(expected[name].shape) for name in ("out", "dx", "dw", "dbias")}
    needed = _native.lib().cusrl_dwconv2d_num_partials(*case["dout"].shape)
    partials = _Guarded((max(needed, 1),), dtype=torch.float64)
    sizes = (*case["x"].shape, *case["geometry"])
    assert _raw(FWD)(inputs["x"].ptr(), inputs["w"].ptr(), inputs["bias"].ptr(), outputs["out"].ptr(), *sizes, _stream()) == 0
    assert _raw(BWD_INPUT)(inputs["dout"].ptr(), inputs["w"].ptr(), outputs["dx"].ptr(), *sizes, _stream()) == 0
    assert _raw(BWD_PARAMS)(inputs["x"].ptr(), inputs["dout"].ptr(), outputs["dw"].ptr(), outputs["dbias"].ptr(), partials.ptr(), *sizes,
                            _stream()) == 0
    torch.cuda.synchronize()
    for name, guarded in [*inputs.items(), *outputs.items(), ("partials", partials)]:
        assert guarded.guards_intact(), f"{name}: a guard float was written"
    assert all(guarded.unchanged() for guarded in inputs.values()), "a read-only operand changed"
    for name, guarded in outputs.items():
        assert not torch.isnan(guarded.tensor).any(), f"{name}: not fully written"
        assert torch.equal(guarded.tensor, expected[name]), name
    if needed:
        assert not torch.isnan(partials.tensor.view(C, -1, 50)[:, :, :case["geometry"][0] * case["geometry"][1]]).any()


def _offset_view(t):
    """The same values one float off a 16-byte boundary."""
    buffer = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("label", ["6x4 k3 p1 no bias", "6x5 k(3,2) p1", "17x16 k7 p3"])
def test_offset_and_channels_last_operands_give_the_bits_of_the_plain_call(cusrl, golden, label):
    case = _on_device(_cnn.kernel_case(golden("cnn"), label, 130, 3))
    assert all(case[name] is None or case[name].data_ptr() % 16 == 0 for name in ("x", "w", "bias", "dout"))
    plain = _forward_backward(case)
    for shifted in [name for name in ("x", "w", "bias", "dout") if case[name] is not None]:
        assert _same(_forward_backward(dict(case, **{shifted: _offset_view(case[shifted])})), plain), f"{shifted} as an offset view"
    strided = dict(case, x=case["x"].contiguous(memory_format=torch.channels_last), dout=case["dout"].contiguous(memory_format=torch.channels_last))
    assert not strided["x"].is_contiguous() and not strided["dout"].is_contiguous()
    staged = _forward_backward(strided)
    assert all(value is None or value.is_contiguous() for value in staged.values()) and _same(staged, plain)


# ------------------------------------------------------------------------------------------------ launch census, modules
@pytest.mark.parametrize("family,name", _cnn.DEVICE_MODULE_CASES)
def test_module_reproduces_the_reference_on_the_device_within_its_launch_budget(cusrl, golden, family, name):
    g = golden("cnn")
    prefix = f"{family}/{name}/"
    module = _cnn.build_module(cusrl, family, name)
    module.load_state_dict(_cnn.recorded_state(g, prefix), strict=True)
    module.to(DEV)
    inputs, w = _cnn.module_inputs(g, family, name)
    layers = 1 if family == "sep" else 2  # SeparableConv2d layers
    before = _counts()
    got = _cnn.run_module(module, inputs, w, DEV)
    assert _delta(before) == (layers, layers, layers), "a gradient asked for on the input and the parameters"
    errors = _cnn.assert_module_matches(prefix + " on the device", got, g, prefix)
    _WORST["modules"] = max(_WORST.get("modules", 0.0), *errors.values())
    device_input = inputs["input"].to(DEV)
    before = _counts()  # an input that wants no gradient: the first layer launches no bwd_input
    output = module(device_input)
    assert _delta(before) == (layers, 0, 0) and torch.equal(output.detach(), got["out"])
    (output * w.to(DEV)).sum().backward()
    assert _delta(before) == (layers, layers - 1, layers)
    for key, parameter in module.named_parameters():
        assert _cnn.relative_to_largest(parameter.grad, g[prefix + "grad/" + key]) <= _cnn.BOUND, key
    with torch.no_grad():  # without a gradient: the forward launches alone, the same output bits
        before = _counts()
        again = module(device_input)
        assert _delta(before) == (layers, 0, 0) and torch.equal(again, got["out"])


def test_worst_module_error_is_printed():
    print(f"worst over every recorded module on the device: {_WORST.get('modules', float('nan')):.3e} of the largest entry")


def test_positional_encodings_on_the_device(cusrl, golden):
    g = golden("cnn")
    for name, ((C, H, W), kwargs) in _cnn.SINUSOIDAL.items():
        layer = cusrl.SinusoidalPositionalEncoding2D(C, H, W, **kwargs).to(DEV)
        assert torch.equal(layer.pe.cpu(), torch.from_numpy(g[f"pe/sinusoidal/{name}/pe"])), "the table is built on the CPU"
        out = layer(torch.from_numpy(g[f"pe/sinusoidal/{name}/x"]).to(DEV))
        assert torch.equal(out.cpu(), torch.from_numpy(g[f"pe/sinusoidal/{name}/out"])), "one rounded fp32 add"
    layer = cusrl.LearnablePositionalEncoding2D(*_cnn.LEARNABLE)
    layer.load_state_dict({"pe": torch.from_numpy(g["pe/learnable/pe"].copy())}, strict=True)
    layer.to(DEV)
    x = torch.from_numpy(g["pe/learnable/x"]).to(DEV)
    out = layer(x)
    assert torch.equal(out.cpu(), torch.from_numpy(g["pe/learnable/out"]))
    out.sum().backward()
    assert torch.equal(layer.pe.grad, torch.full_like(layer.pe, 2.0))  # (the batch of 2 broadcast onto the table)


# ------------------------------------------------------------------------------------------------ fallbacks
def test_fallback_predicates(cusrl, golden):
    """Predicate calls only: no convolution runs on the device and no counter moves."""
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    case = _on_device(_cnn.kernel_case(golden("cnn"), "17x16 k7 p3", 3, 3))
    x, w, bias = case["x"], case["w"], case["bias"]
    before = _counts()
    assert ops.dwconv2d_supported(x, w, bias, 1, 3, 1) and ops.dwconv2d_supported(x, w, None, (1, 1), (3, 3), (1, 1), "zeros")
    with torch.autocast("cuda"):
        assert not ops.dwconv2d_supported(x, w, bias, 1, 3, 1)
    assert not ops.dwconv2d_supported(x.double(), w.double(), bias.double(), 1, 3, 1)
    assert not ops.dwconv2d_supported(x, w.double(), bias, 1, 3, 1) and not ops.dwconv2d_supported(x.cpu(), w, bias, 1, 3, 1)
    with double_differentiable():
        assert not ops.dwconv2d_supported(x.clone().requires_grad_(True), w, bias, 1, 3, 1)
        assert not ops.dwconv2d_supported(x, w.clone().requires_grad_(True), bias, 1, 3, 1)
        assert ops.dwconv2d_supported(x, w, bias, 1, 3, 1), "nothing asks for a gradient"
        with torch.no_grad():
            assert ops.dwconv2d_supported(x.clone().requires_grad_(True), w, bias, 1, 3, 1)
    assert not ops.dwconv2d_supported(x, w, bias, 1, 3, 1, "reflect") and not ops.dwconv2d_supported(x, w, bias, 1, 3, 1, "circular")
    wide = torch.zeros(3, 1, 8, 8, device=DEV)
    assert not ops.dwconv2d_supported(x, wide, bias, 1, 4, 1), "64 taps"
    assert ops.dwconv2d_supported(x, w, bias, 1, "same", 1) and ops.dwconv2d_supported(x, w, bias, 1, "valid", 1)
    even = torch.zeros(3, 1, 4, 4, device=DEV)
    assert not ops.dwconv2d_supported(x, even, bias, 1, "same", 1), "an asymmetric 'same': D (K - 1) is odd"
    assert ops.dwconv2d_supported(x, even, bias, 1, "same", 2) and not ops.dwconv2d_supported(x, w, bias, 2, "same", 1)
    assert not ops.dwconv2d_supported(x, torch.zeros(6, 1, 3, 3, device=DEV), None, 1, 1, 1), "a channel multiplier"
    assert not ops.dwconv2d_supported(x, w, bias, 1, 0, 3), "no output: D (K - 1) = 18 rows of a 17-row image"
    assert _delta(before) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ an agent
def test_agent_with_a_cnn_backbone_trains(cusrl):
    """``Cnn([SeparableConv2d, ReLU, SeparableConv2d])`` through ``Cnn.Factory`` as the actor's backbone in the eager ``ppo``
    preset: 8 envs with 6 x 6 observations, 4 steps per update, 2 epochs x 2 minibatches, 2 iterations."""

    class Census(cusrl.Hook):
        def __init__(self):
            super().__init__()
            self.marks = []

        def pre_update(self, buffer):
            self.marks.append(_counts())

        def post_update(self):
            self.marks.append(_counts())

    Sep = cusrl.SeparableConv2d
    cusrl.set_global_seed(13)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=36, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=4, sampler_epochs=2, sampler_mini_batches=2).to_underlying()
    factory.actor_factory.backbone_factory = cusrl.Cnn.Factory(
        [lambda: Sep(1, 4, 3, padding=1), torch.nn.ReLU, lambda: Sep(4, 4, 3, stride=2)], input_shape=(6, 6))
    factory.actor_factory.latent_dim = 16
    census = Census()
    factory.register_hook(census)
    trainer = cusrl.Trainer(env, factory, num_iterations=2, verbose=False)
    agent = trainer.agent
    backbone = agent.actor.backbone
    assert isinstance(backbone, cusrl.Cnn) and (backbone.input_dim, backbone.output_dim) == (36, 16)
    assert [type(layer).__name__ for layer in backbone.layers] == ["SeparableConv2d", "ReLU", "SeparableConv2d", "Flatten", "Linear"]
    initial = {name: param.detach().clone() for name, param in agent.named_parameters()}
    start = _counts()
    trainer.run_training_loop()
    torch.cuda.synchronize()
    assert len(census.marks) == 4  # pre_update, post_update, twice
    marks = [start, *census.marks]
    rollouts = [tuple(b - a for a, b in zip(marks[i], marks[i + 1])) for i in (0, 2)]
    updates = [tuple(b - a for a, b in zip(marks[i], marks[i + 1])) for i in (1, 3)]
    print(f"(fwd, bwd_input, bwd_params) launches: rollouts {rollouts}, updates {updates}")
    for fwd, bwd_input, bwd_params in rollouts:
        assert fwd >= 2 * 4 and (bwd_input, bwd_params) == (0, 0), "both layers' forward launch per act step, no backward"
    for fwd, bwd_input, bwd_params in updates:
        steps = 2 * 2
        assert fwd >= 2 * steps and bwd_params == 2 * steps, "both layers per minibatch step"
        assert bwd_input == steps, "the first layer reads observations: only the second launches bwd_input"
    assert np.isfinite(trainer.last_info["Agent/value_loss"])
    for key in ("Agent/surrogate_loss", "Agent/kl_divergence"):
        if key in trainer.last_info:
            assert np.isfinite(trainer.last_info[key]), key
    for name, param in agent.named_parameters():
        assert torch.isfinite(param).all(), name
        if param.requires_grad:
            assert not torch.equal(param, initial[name]), f"{name} did not change"
