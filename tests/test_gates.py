"""Gate layers, GLU activations and FeedForward without a GPU: the public surface, the reference's recorded state dicts and runs
(golden ``gates.npz``), the torch-expression path that CPU tensors take, and the kernel formulas restated in float32 against
their float64 evaluation under the assertions the GPU tests use."""

from __future__ import annotations

import itertools

import pytest
import torch

import _gates

GATE_NAMES = ["Gate", "GruGate", "HighwayGate", "InputGate", "OutputGate", "PassthroughGate", "ResidualGate", "SigmoidTanhGate", "get_gate_cls"]
NAMES = [*GATE_NAMES, "GeGlu", "SwiGlu", "FeedForward"]
SYMBOLS = {"cusrl_gate_fwd", "cusrl_gate_bwd", "cusrl_glu_fwd", "cusrl_glu_bwd"}
INITIAL_BIASES = {("output", "gate_linear.bias"): -1.0, ("highway", "gate_linear.bias"): 1.0, ("sigmoid_tanh", "sigmoid_linear.bias"): -1.0,
                  ("gru", "z_x.bias"): -2.0}
STATE_KEYS = {
    "passthrough": [], "residual": [], "input": ["gate_linear.weight"], "output": ["gate_linear.weight", "gate_linear.bias"],
    "highway": ["gate_linear.weight", "gate_linear.bias"],
    "sigmoid_tanh": ["sigmoid_linear.weight", "sigmoid_linear.bias", "tanh_linear.weight"],
    "gru": ["r_y.weight", "r_x.weight", "z_y.weight", "z_x.weight", "z_x.bias", "h_y.weight", "h_rx.weight"],
}


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def _launches():
    from cusrl_amd import _native

    return {symbol: _native.launch_counts.get(symbol, 0) for symbol in SYMBOLS}


def test_names_are_exported_from_both_namespaces(cusrl):
    import cusrl_amd.nn.activation
    import cusrl_amd.nn.feedforward
    import cusrl_amd.nn.gate

    for namespace in (cusrl, cusrl.nn):
        assert set(NAMES) <= set(namespace.__all__)
        for name in NAMES:
            assert getattr(namespace, name) is getattr(cusrl.nn, name)
    for name in GATE_NAMES:
        assert getattr(cusrl.nn.gate, name) is getattr(cusrl, name) and name in cusrl.nn.gate.__all__
    assert cusrl.nn.activation.GeGlu is cusrl.GeGlu and cusrl.nn.activation.SwiGlu is cusrl.SwiGlu
    assert cusrl.nn.feedforward.FeedForward is cusrl.FeedForward
    assert issubclass(cusrl.GeGlu, torch.nn.GLU) and issubclass(cusrl.SwiGlu, torch.nn.GLU)
    assert cusrl.GeGlu().dim == -1 and cusrl.SwiGlu(dim=0).dim == 0
    for name in ("gate_combine", "gate_supported", "glu", "glu_supported", "GateCombine", "Glu"):
        assert hasattr(cusrl_amd.ops, name), name


def test_abi_stays_7_and_the_new_symbols_are_bound(cusrl):
    from cusrl_amd import _native

    assert _native.ABI_VERSION == 7
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    assert [_native._CONSTANTS["GATE_" + kind.upper()] for kind in _gates.GATE_KINDS] == [0, 1, 2, 3, 4, 5]
    assert (_native._CONSTANTS["GLU_GEGLU"], _native._CONSTANTS["GLU_SWIGLU"]) == (0, 1)
    lib = _native.lib()  # argument validation runs on the host: no device is touched
    invalid = _native._CONSTANTS["E_INVALID"]
    assert lib.cusrl_gate_fwd(0, None, None, None, None, None, None, None, 3, 4, None) == invalid
    assert lib.cusrl_glu_bwd(0, None, None, None, 3, 4, None) == invalid


def test_get_gate_cls_covers_the_map_and_names_what_it_refuses(cusrl):
    from cusrl_amd.nn.gate import gate_map

    assert list(gate_map) == [None, "gru", "highway", "input", "output", "residual", "sigmoid_tanh"]
    for name, gate_type in _gates.GATE_TYPES.items():
        cls = cusrl.get_gate_cls(gate_type)
        assert cls is gate_map[gate_type] and issubclass(cls, cusrl.Gate) and cls(8).embed_dim == 8, name
    with pytest.raises(ValueError) as raised:
        cusrl.get_gate_cls("lstm")
    assert str(raised.value) == ("Unsupported gate type 'lstm'; available gate types: None, 'gru', 'highway', 'input', 'output', "
                                 "'residual', 'sigmoid_tanh'")
    with pytest.raises(NotImplementedError):
        cusrl.Gate(4)(torch.zeros(1, 4), torch.zeros(1, 4))


@pytest.mark.parametrize("family,name,size", _gates.MODULE_CASES)
def test_state_dict_is_the_references(cusrl, golden, family, name, size):
    """Keys in the reference's order, the initial bias fills, shapes, and a strict load of the recorded state."""
    g = golden("gates")
    prefix = _gates.module_prefix(family, name, size)
    torch.manual_seed(0)
    module = _gates.build_module(cusrl, family, name, size)
    recorded = _gates.recorded_state(g, prefix)
    assert list(module.state_dict()) == list(recorded) == [str(key) for key in g[prefix + "state_keys"]]
    if family == "gate":
        assert list(recorded) == STATE_KEYS[name]
    for key, value in module.state_dict().items():
        assert value.shape == recorded[key].shape and value.dtype == recorded[key].dtype, key
        if (name, key) in INITIAL_BIASES and family == "gate":
            fill = torch.full_like(value, INITIAL_BIASES[name, key])
            assert torch.equal(value, fill) and torch.equal(recorded[key], fill), key
    result = module.load_state_dict(recorded, strict=True)
    assert not result.missing_keys and not result.unexpected_keys


def test_feedforward_layers_and_widths(cusrl):
    ff = cusrl.FeedForward(6, 16, cusrl.GeGlu)
    assert [type(layer).__name__ for layer in ff.layers] == ["Linear", "GeGlu", "Linear"]
    assert (ff.input_dim, ff.feedforward_dim, ff.output_dim) == (6, 16, 6) and ff.layers[2].in_features == 8  # the GLU halves 16
    ff = cusrl.FeedForward(8, 16, cusrl.SwiGlu, dropout=0.25, output_dim=4)
    assert [type(layer).__name__ for layer in ff.layers] == ["Linear", "SwiGlu", "Dropout", "Linear"]
    assert list(ff.state_dict()) == ["layers.0.weight", "layers.0.bias", "layers.3.weight", "layers.3.bias"]
    assert ff.layers[3].in_features == 8 and ff.layers[3].out_features == 4 and ff.layers[2].p == 0.25
    ff = cusrl.FeedForward(6)
    assert [type(layer).__name__ for layer in ff.layers] == ["Linear", "GELU", "Linear"]
    assert (ff.feedforward_dim, ff.output_dim, ff.layers[2].in_features) == (24, 6, 24)


@pytest.mark.parametrize("family,name,size", _gates.MODULE_CASES)
def test_module_reproduces_the_reference(cusrl, golden, family, name, size):
    g = golden("gates")
    prefix = _gates.module_prefix(family, name, size)
    module = _gates.build_module(cusrl, family, name, size)
    module.load_state_dict(_gates.recorded_state(g, prefix), strict=True)
    inputs, w = _gates.module_inputs(g, family, name, size)
    before = _launches()
    got = _gates.run_module(module, inputs, w)
    assert _launches() == before, "a CPU tensor launches nothing"
    _gates.assert_module_matches(prefix, got, g, prefix)


def test_cpu_tensors_are_not_supported_and_take_the_torch_expression(cusrl, golden):
    from cusrl_amd import ops

    g = golden("gates")
    before = _launches()
    for kind in _gates.GATE_KINDS:
        case = _gates.gate_case(g, kind, 3, 4, second=True)
        operands = [case[name] for name in ("x", "y", "p", "q", "p2", "q2")]
        assert not ops.gate_supported(kind, *operands)
        out = ops.gate_combine(kind, *operands)
        want = _gates.gate_formulas(kind, case, torch.float64)["out"]
        assert out.dtype == torch.float32 and _gates.relative_to_largest(out, want) <= _gates.BOUND
    for kind in _gates.GLU_KINDS:
        case = _gates.glu_case(g, 3, 4)
        assert not ops.glu_supported(case["input"]) and not ops.glu_supported(case["input"], 0)
        out = ops.glu(kind, case["input"])
        assert _gates.relative_to_largest(out, _gates.glu_formulas(kind, case, torch.float64)["out"]) <= _gates.BOUND
        tall = _gates.glu_case(g, 4, 4)["input"]  # [4, 8] split along dim 0
        top, bottom = tall.chunk(2, dim=0)
        act = torch.nn.functional.gelu if kind == "geglu" else torch.nn.functional.silu
        assert torch.equal(ops.glu(kind, tall, dim=0), top * act(bottom))
    assert _launches() == before
    with pytest.raises(ValueError, match="Unknown gate kind 'lstm'"):
        ops.gate_combine("lstm", torch.zeros(1), torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match="needs x, p, q"):
        ops.gate_combine("gru_out", torch.zeros(1), None, torch.zeros(1))
    with pytest.raises(ValueError, match="Unknown GLU kind 'reglu'"):
        ops.glu("reglu", torch.zeros(2))


# ------------------------------------------------------------------------------------------------ the formulas in float32
@pytest.mark.parametrize("kind,rows,C", list(itertools.product(_gates.GATE_KINDS, _gates.ROWS, _gates.WIDTHS)))
def test_float32_restatement_of_the_gate_formulas_meets_the_gpu_bounds(golden, kind, rows, C):
    """The assertions of tests/test_gates_gpu.py on its cases, with torch's CPU float32 in the kernel's place."""
    case = _gates.gate_case(golden("gates"), kind, rows, C)
    want = _gates.gate_formulas(kind, case, torch.float64)
    assert sorted(want) == sorted(("out", *_gates.GRADIENTS[kind]))
    _gates.assert_kernel_matches(f"float32 {kind} [{rows}, {C}]", _gates.gate_formulas(kind, case, torch.float32, kernel_order=True), want)


def test_why_the_backward_does_not_subtract_in_float32(golden):
    """``1 - g`` and ``1 - h h`` as rounded fp32 differences lose the bound on a tensor whose largest entry sits where the
    activation is close to saturation (a gradient tensor of a handful of entries); the kernel's route does not."""
    case = _gates.gate_case(golden("gates"), "gru_out", 1, 1)
    want = _gates.gate_formulas("gru_out", case, torch.float64)
    naive = _gates.gate_formulas("gru_out", case, torch.float32)
    assert _gates.relative_to_largest(naive["dq"], want["dq"].numpy()) > _gates.BOUND
    assert _gates.relative_to_largest(_gates.gate_formulas("gru_out", case, torch.float32, kernel_order=True)["dq"], want["dq"].numpy()) <= _gates.BOUND


@pytest.mark.parametrize("kind,rows,H", list(itertools.product(_gates.GLU_KINDS, _gates.ROWS, _gates.WIDTHS)))
def test_float32_restatement_of_the_glu_formulas_meets_the_gpu_bounds(golden, kind, rows, H):
    case = _gates.glu_case(golden("gates"), rows, H)
    _gates.assert_kernel_matches(f"float32 {kind} [{rows}, 2 x {H}]", _gates.glu_formulas(kind, case, torch.float32),
                                 _gates.glu_formulas(kind, case, torch.float64))


def test_float32_restatement_of_the_saturated_cases(golden):
    g = golden("gates")
    for kind in _gates.GATE_KINDS:
        case = _gates.saturated_gate_case(g, kind)
        masks = _gates.saturation_masks(kind, case)
        assert masks["dp"].sum() >= 12, "sigmoid is exactly 0 or 1 at +-100 and at +20"
        _gates.assert_saturated(f"float32 saturated {kind}", _gates.gate_formulas(kind, case, torch.float32, kernel_order=True),
                                _gates.gate_formulas(kind, case, torch.float64), masks)
    for kind in _gates.GLU_KINDS:
        case = _gates.saturated_glu_case(g)
        _gates.assert_saturated(f"float32 saturated {kind}", _gates.glu_formulas(kind, case, torch.float32),
                                _gates.glu_formulas(kind, case, torch.float64))


def test_the_formulas_are_the_gradients_of_the_forward(golden):
    """The float64 evaluation the kernels are held to is autograd's gradient of its own forward."""
    g = golden("gates")
    for kind in _gates.GATE_KINDS:
        case = _gates.gate_case(g, kind, 3, 5)
        leaves = {name: None if value is None else value.double().requires_grad_(name != "dout") for name, value in case.items()}
        out = _gates.gate_formulas(kind, {**leaves, "dout": case["dout"]}, torch.float64)["out"]
        wanted = {"dx": "x", "dy": "y", "dp": "p", "dq": "q"}
        names = _gates.GRADIENTS[kind]
        grads = torch.autograd.grad(out, [leaves[wanted[name]] for name in names], grad_outputs=case["dout"].double())
        formulas = _gates.gate_formulas(kind, case, torch.float64)
        for name, grad in zip(names, grads):
            assert torch.allclose(grad, formulas[name], rtol=1e-12, atol=1e-14), (kind, name)
        if case["p2"] is not None:  # the second addend's gradient is dp
            (dp2,) = torch.autograd.grad(_gates.gate_formulas(kind, {**leaves, "dout": case["dout"]}, torch.float64)["out"], leaves["p2"],
                                         grad_outputs=case["dout"].double())
            assert torch.allclose(dp2, formulas["dp"], rtol=1e-12, atol=1e-14)
    for kind in _gates.GLU_KINDS:
        case = _gates.glu_case(g, 3, 5)
        leaf = case["input"].double().requires_grad_(True)
        out = _gates.glu_formulas(kind, {"input": leaf, "dout": case["dout"]}, torch.float64)["out"]
        (grad,) = torch.autograd.grad(out, leaf, grad_outputs=case["dout"].double())
        assert torch.allclose(grad, _gates.glu_formulas(kind, case, torch.float64)["dinput"], rtol=1e-12, atol=1e-14), kind
        gelu = torch.nn.functional.gelu if kind == "geglu" else torch.nn.functional.silu
        a, b = case["input"].double().chunk(2, dim=-1)
        assert torch.allclose(out, a * gelu(b), rtol=1e-12, atol=1e-14), "the reference's expression"
