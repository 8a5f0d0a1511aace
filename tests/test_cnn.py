"""Cnn, SeparableConv2d and the 2-D positional encodings without a GPU: the public surface, the host-side validation of the
depthwise-convolution entries, the reference's recorded state dicts and runs (golden ``cnn.npz``), the torch path that CPU
tensors take, and the kernel formulas restated in float32 against their float64 evaluation under the assertions the GPU tests
use."""

from __future__ import annotations

import pytest
import torch

import _cnn

NAMES = ["Cnn", "CnnFactory", "SeparableConv2d", "SinusoidalPositionalEncoding2D", "LearnablePositionalEncoding2D"]
GOOD = (2, 3, 5, 7, 3, 3, 1, 1, 0, 0, 1, 1)  # N, C, H, W, KH, KW, SH, SW, PH, PW, DH, DW
POINTER = 4096  # (a non-NULL address: validation never dereferences, and nothing that passes it here reaches a launch)


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def _launches():
    from cusrl_amd import _native

    return dict(_native.launch_counts)


@pytest.fixture(autouse=True)
def no_launch_counter_moves(cusrl):
    """Nothing in this file launches: the raw ctypes calls below are not counted, and every tensor lives on the CPU."""
    before = _launches()
    yield
    assert _launches() == before, "a launch counter moved in a test without a GPU"


def test_names_are_exported_from_both_namespaces(cusrl):
    import cusrl_amd.nn.cnn
    import cusrl_amd.nn.encoding2d
    import cusrl_amd.nn.separable_conv
    from cusrl_amd import ops

    for namespace in (cusrl, cusrl.nn):
        assert set(NAMES) <= set(namespace.__all__)
        for name in NAMES:
            assert getattr(namespace, name) is getattr(cusrl.nn, name)
    assert cusrl.Cnn is cusrl.nn.cnn.Cnn and cusrl.CnnFactory is cusrl.nn.cnn.CnnFactory and cusrl.Cnn.Factory is cusrl.CnnFactory
    assert cusrl.SeparableConv2d is cusrl.nn.separable_conv.SeparableConv2d
    assert cusrl.SinusoidalPositionalEncoding2D is cusrl.nn.encoding2d.SinusoidalPositionalEncoding2D
    assert cusrl.LearnablePositionalEncoding2D is cusrl.nn.encoding2d.LearnablePositionalEncoding2D
    assert set(cusrl.nn.encoding2d.__all__) == {"LearnablePositionalEncoding2D", "SinusoidalPositionalEncoding2D",
                                                "sinusoidal_positional_encoding_2d"}
    assert issubclass(cusrl.Cnn, cusrl.Module) and issubclass(cusrl.CnnFactory, cusrl.ModuleFactory)
    assert cusrl.Cnn.batch_invariant is False
    for name in ("dwconv2d_supported", "depthwise_conv2d", "DepthwiseConv2d", "dwconv2d_backward_input", "dwconv2d_backward_params"):
        assert hasattr(ops, name), name


def test_abi_stays_7_and_the_new_symbols_are_bound(cusrl):
    from cusrl_amd import _native

    assert _native.ABI_VERSION == 7
    assert set(_cnn.SYMBOLS) <= set(_native.EXPORTED_SYMBOLS)
    assert _native._CONSTANTS["MAX_DWCONV_TAPS"] == _native.MAX_DWCONV_TAPS == 49
    lib = _native.lib()
    for symbol in _cnn.SYMBOLS:
        assert hasattr(lib, symbol), symbol
    assert len(_native._PROTOTYPES["cusrl_dwconv2d_fwd"][1]) == 4 + 12 + 1
    assert len(_native._PROTOTYPES["cusrl_dwconv2d_bwd_input"][1]) == 3 + 12 + 1
    assert len(_native._PROTOTYPES["cusrl_dwconv2d_bwd_params"][1]) == 5 + 12 + 1


def _replaced(index: int, value: int) -> tuple:
    sizes = list(GOOD)
    sizes[index] = value
    return tuple(sizes)


INVALID_SIZES = {
    "N < 0": _replaced(0, -1), "C < 1": _replaced(1, 0), "H < 1": _replaced(2, 0), "W < 1": _replaced(3, 0), "KH < 1": _replaced(4, 0),
    "KW < 1": _replaced(5, 0), "SH < 1": _replaced(6, 0), "SW < 1": _replaced(7, 0), "PH < 0": _replaced(8, -1), "PW < 0": _replaced(9, -1),
    "DH < 1": _replaced(10, 0), "DW < 1": _replaced(11, 0),
    "Ho < 1": (2, 3, 5, 7, 3, 3, 1, 1, 0, 0, 3, 1),  # D (K - 1) = 6 rows of a 5-row image
    "Wo < 1": (2, 3, 5, 2, 3, 3, 1, 1, 0, 0, 1, 1),
}
UNSUPPORTED_SIZES = {
    "64 taps": (2, 3, 9, 9, 8, 8, 1, 1, 0, 0, 1, 1),
    "50 taps": (2, 3, 60, 9, 50, 1, 1, 1, 0, 0, 1, 1),
    "N C H W beyond int64": (2 ** 40, 2 ** 20, 2 ** 10, 2 ** 10, 3, 3, 1, 1, 0, 0, 1, 1),
    "2 P + H beyond int64": (2, 3, 5, 7, 3, 3, 1, 1, 2 ** 62, 0, 1, 1),
}


def _calls(lib, sizes):
    """The three entries on these sizes with every pointer present: ``{label: status}``."""
    P = POINTER
    return {"fwd": lib.cusrl_dwconv2d_fwd(P, P, P, P, *sizes, None), "bwd_input": lib.cusrl_dwconv2d_bwd_input(P, P, P, *sizes, None),
            "bwd_params": lib.cusrl_dwconv2d_bwd_params(P, P, P, P, P, *sizes, None)}


@pytest.mark.parametrize("row", list(INVALID_SIZES))
def test_invalid_sizes_are_refused_on_the_host(cusrl, row):
    from cusrl_amd import _native

    assert set(_calls(_native.lib(), INVALID_SIZES[row]).values()) == {_native._CONSTANTS["E_INVALID"]}, row


@pytest.mark.parametrize("row", list(UNSUPPORTED_SIZES))
def test_unsupported_sizes_are_refused_on_the_host(cusrl, row):
    from cusrl_amd import _native

    assert set(_calls(_native.lib(), UNSUPPORTED_SIZES[row]).values()) == {_native._CONSTANTS["E_UNSUPPORTED"]}, row
    assert _native._CONSTANTS["E_UNSUPPORTED"] != _native._CONSTANTS["E_INVALID"]


def test_null_pointers_are_refused_and_an_empty_batch_is_a_no_op(cusrl):
    from cusrl_amd import _native

    lib, invalid, P = _native.lib(), _native._CONSTANTS["E_INVALID"], POINTER
    for missing in (0, 1, 3):  # x, w, out (bias, the third, is optional)
        pointers = [P, P, P, P]
        pointers[missing] = None
        assert lib.cusrl_dwconv2d_fwd(*pointers, *GOOD, None) == invalid, missing
    for missing in range(3):  # dout, w, dx
        pointers = [P, P, P]
        pointers[missing] = None
        assert lib.cusrl_dwconv2d_bwd_input(*pointers, *GOOD, None) == invalid, missing
    for missing in range(3):  # x, dout, dw (dbias is optional; partials where num_partials > 0)
        pointers = [P, P, P, P, P]
        pointers[missing] = None
        assert lib.cusrl_dwconv2d_bwd_params(*pointers, *GOOD, None) == invalid, missing
    many = (130, 3, 17, 16, 7, 7, 1, 1, 3, 3, 1, 1)
    assert lib.cusrl_dwconv2d_num_partials(130, 3, 17, 16) > 1 and lib.cusrl_dwconv2d_bwd_params(P, P, P, P, None, *many, None) == invalid
    empty = (0, *GOOD[1:])
    assert set(_calls(lib, empty).values()) == {0}, "N == 0 is a successful no-op"
    assert lib.cusrl_dwconv2d_fwd(P, P, None, P, *empty, None) == 0 and lib.cusrl_dwconv2d_bwd_params(P, P, P, None, None, *empty, None) == 0


def test_num_partials(cusrl):
    from cusrl_amd import _native

    partials = _native.lib().cusrl_dwconv2d_num_partials
    assert partials(1, 1, 1, 1) == 0 and partials(4, 3, 16, 16) == 0, "one block per channel covers 1024 positions"
    assert partials(4, 3, 16, 16 + 1) == 3 * 2 * 50 and partials(130, 3, 17, 16) == 3 * 35 * 50
    assert partials(10 ** 6, 2, 17, 16) == 2 * 64 * 50, "at most 64 blocks per channel"
    assert partials(0, 3, 5, 7) == 0 and partials(2, 3, 0, 7) == 0 and partials(2 ** 40, 3, 2 ** 20, 2 ** 10) == -1


# ------------------------------------------------------------------------------------------------ recorded modules
@pytest.mark.parametrize("family,name", _cnn.MODULE_CASES)
def test_state_dict_is_the_references(cusrl, golden, family, name):
    """Keys in the reference's order, shapes, dtypes, and a strict load of the recorded state."""
    g = golden("cnn")
    prefix = f"{family}/{name}/"
    torch.manual_seed(0)
    module = _cnn.build_module(cusrl, family, name)
    recorded = _cnn.recorded_state(g, prefix)
    assert list(module.state_dict()) == list(recorded) == [str(key) for key in g[prefix + "state_keys"]]
    for key, value in module.state_dict().items():
        assert value.shape == recorded[key].shape and value.dtype == recorded[key].dtype, key
    result = module.load_state_dict(recorded, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    if family == "sep":
        bias = _cnn.SEPARABLE[name][3].get("bias", True)
        keys = ["depthwise.weight", "depthwise.bias", "pointwise.weight", "pointwise.bias"] if bias else ["depthwise.weight", "pointwise.weight"]
        assert list(recorded) == keys
        assert isinstance(module.depthwise, torch.nn.Conv2d) and module.depthwise.groups == module.depthwise.in_channels
        assert isinstance(module.pointwise, torch.nn.Conv2d) and module.pointwise.kernel_size == (1, 1)
    else:
        assert all(key.startswith("layers.") for key in recorded)
        assert (module.input_dim, module.output_dim) == tuple(g[f"cnn_dims/{name}"])


def test_default_initialisation_is_the_references(cusrl, golden):
    """Under the recording's seed the constructor draws the recorded parameters: the same sub-modules, built in the same order."""
    g = golden("cnn")
    for index, name in enumerate(_cnn.SEPARABLE):
        torch.manual_seed(7100 + index)
        module = _cnn.build_module(cusrl, "sep", name)
        for key, value in _cnn.recorded_state(g, f"sep/{name}/").items():
            assert torch.equal(module.state_dict()[key], value), (name, key)


@pytest.mark.parametrize("family,name", _cnn.MODULE_CASES)
def test_module_reproduces_the_reference(cusrl, golden, family, name):
    g = golden("cnn")
    prefix = f"{family}/{name}/"
    module = _cnn.build_module(cusrl, family, name)
    module.load_state_dict(_cnn.recorded_state(g, prefix), strict=True)
    inputs, w = _cnn.module_inputs(g, family, name)
    _cnn.assert_module_matches(prefix, _cnn.run_module(module, inputs, w), g, prefix)


def test_cnn_dims_layers_and_error_texts(cusrl):
    Sep = cusrl.SeparableConv2d
    layers = lambda: [Sep(1, 4, 3, padding=1), torch.nn.ReLU(), Sep(4, 4, 3, stride=2)]  # noqa: E731
    cnn = cusrl.Cnn(layers(), input_shape=(6, 6), output_dim=16)
    assert (cnn.input_dim, cnn.output_dim, cnn.input_shape, cnn.input_flattened) == (36, 16, (1, 6, 6), True)
    assert [type(layer).__name__ for layer in cnn.layers] == ["SeparableConv2d", "ReLU", "SeparableConv2d", "Flatten", "Linear"]
    assert cnn.layers[3].start_dim == -3 and cnn.layers[4].in_features == 4 * 2 * 2
    assert cnn(torch.zeros(36)).shape == (16,) and cnn(torch.zeros(7, 5, 3, 36)).shape == (7, 5, 3, 16)
    cnn = cusrl.Cnn(layers(), input_shape=(1, 6, 6), input_flattened=False)
    assert (cnn.input_dim, cnn.output_dim) == (36, 16) and type(cnn.layers[-1]).__name__ == "Flatten"
    assert cnn(torch.zeros(1, 6, 6)).shape == (16,) and cnn(torch.zeros(2, 3, 1, 6, 6)).shape == (2, 3, 16)
    cnn = cusrl.Cnn(layers(), input_shape=(6, 6), flatten_output=False)
    assert cnn.output_dim == 16 and len(cnn.layers) == 3 and cnn(torch.zeros(5, 36)).shape == (5, 4, 2, 2)
    with pytest.raises(ValueError) as raised:
        cusrl.Cnn(layers(), input_shape=(6,))
    assert str(raised.value) == "'input_shape' must be 2D or 3D"
    with pytest.raises(ValueError) as raised:
        cusrl.Cnn(layers(), input_shape=(6, 6), flatten_output=False, output_dim=16)
    assert str(raised.value) == "'flatten_output' must be True if 'output_dim' is set"
    factory = cusrl.Cnn.Factory([lambda: Sep(1, 4, 3, padding=1), torch.nn.ReLU, lambda: Sep(4, 4, 3, stride=2)], input_shape=(6, 6))
    built = factory(36, 16)
    assert isinstance(built, cusrl.Cnn) and (built.input_dim, built.output_dim) == (36, 16) and factory().output_dim == 16
    with pytest.raises(ValueError) as raised:
        factory(35, 16)
    assert str(raised.value) == "Input dimension mismatch: expected 36, got 35"


# ------------------------------------------------------------------------------------------------ positional encodings
def test_positional_encodings_are_the_references(cusrl, golden):
    from cusrl_amd.nn.encoding2d import sinusoidal_positional_encoding_2d

    g = golden("cnn")
    for name, ((C, H, W), kwargs) in _cnn.SINUSOIDAL.items():
        layer = cusrl.SinusoidalPositionalEncoding2D(C, H, W, **kwargs)
        recorded = torch.from_numpy(g[f"pe/sinusoidal/{name}/pe"])
        assert layer.pe.shape == (C, H, W) and torch.equal(layer.pe, recorded), f"{name}: not the recorded bits"
        assert isinstance(layer.pe, torch.nn.Parameter) and layer.pe.requires_grad == bool(g[f"pe/sinusoidal/{name}/requires_grad"]) is False
        assert list(layer.state_dict()) == ["pe"]
        assert torch.equal(layer(torch.from_numpy(g[f"pe/sinusoidal/{name}/x"])), torch.from_numpy(g[f"pe/sinusoidal/{name}/out"]))
        table = sinusoidal_positional_encoding_2d(H, W, C, **kwargs)
        assert table.shape == (H, W, C) and torch.equal(table.permute(2, 0, 1), recorded)
    assert cusrl.SinusoidalPositionalEncoding2D(4, 2, 2, requires_grad=True).pe.requires_grad
    with pytest.raises(ValueError) as raised:
        cusrl.SinusoidalPositionalEncoding2D(6, 2, 2)
    assert str(raised.value) == "'num_channels' must be divisible by 4 for 2D sinusoidal encoding; got 6"
    torch.manual_seed(int(g["pe/learnable/seed"]))
    layer = cusrl.LearnablePositionalEncoding2D(*_cnn.LEARNABLE)
    assert torch.equal(layer.pe, torch.from_numpy(g["pe/learnable/pe"])), "trunc_normal_(std=0.02) under the recorded seed"
    assert layer.pe.requires_grad == bool(g["pe/learnable/requires_grad"]) is True
    assert torch.equal(layer(torch.from_numpy(g["pe/learnable/x"])), torch.from_numpy(g["pe/learnable/out"]))
    assert layer(torch.zeros(3, 2, *_cnn.LEARNABLE, dtype=torch.float64)).dtype == torch.float64  # (pe.type_as(x))


# ------------------------------------------------------------------------------------------------ the torch path
def test_cpu_tensors_are_not_supported_and_take_torchs_convolution(cusrl, golden):
    from cusrl_amd import ops

    g = golden("cnn")
    for label in ("5x7 k3", "33x9 k(5,3) s(2,1) p(2,3) d(2,1)", "6x4 k3 p1 no bias"):
        case = _cnn.kernel_case(g, label, 3, 3)
        KH, KW, SH, SW, PH, PW, DH, DW = case["geometry"]
        arguments = (case["x"], case["w"], case["bias"], (SH, SW), (PH, PW), (DH, DW))
        assert not ops.dwconv2d_supported(*arguments) and not ops.dwconv2d_supported(*arguments, "zeros")
        out = ops.depthwise_conv2d(*arguments)
        assert torch.equal(out, torch.nn.functional.conv2d(*arguments, groups=3))
        assert _cnn.relative_to_largest(out, _cnn.dwconv_formulas(case, torch.float64)["out"].numpy()) <= _cnn.BOUND


# ------------------------------------------------------------------------------------------------ the formulas in float32
@pytest.mark.parametrize("label,N,C", _cnn.KERNEL_CASES)
def test_float32_restatement_of_the_formulas_meets_the_gpu_bounds(golden, label, N, C):
    """The assertions of tests/test_cnn_gpu.py on its cases, with torch's CPU float32 in the kernel's place."""
    case = _cnn.kernel_case(golden("cnn"), label, N, C)
    _cnn.assert_kernel_matches(f"float32 {label} [{N}, {C}]", _cnn.dwconv_formulas(case, torch.float32), case)


def test_the_formulas_are_torchs_convolution_and_its_gradients(golden):
    """The float64 evaluation the kernels are held to is torch's depthwise convolution and autograd's gradients of it."""
    g = golden("cnn")
    for label in _cnn.GEOMETRIES:
        case = _cnn.kernel_case(g, label, 3, 3)
        KH, KW, SH, SW, PH, PW, DH, DW = case["geometry"]
        leaves = [None if case[name] is None else case[name].double().requires_grad_(True) for name in ("x", "w", "bias")]
        out = torch.nn.functional.conv2d(*leaves, (SH, SW), (PH, PW), (DH, DW), groups=3)
        present = [leaf for leaf in leaves if leaf is not None]
        grads = iter(torch.autograd.grad(out, present, grad_outputs=case["dout"].double()))
        formulas = _cnn.dwconv_formulas(case, torch.float64)
        assert torch.allclose(out, formulas["out"], rtol=1e-12, atol=1e-13), label
        for name, leaf in zip(("dx", "dw", "dbias"), leaves):
            if leaf is not None:
                assert torch.allclose(next(grads), formulas[name], rtol=1e-12, atol=1e-12), (label, name)
    unread = _cnn.unread_positions(_cnn.kernel_case(g, "8x8 k3 s2", 1, 1))
    assert unread[7].all() and unread[:, 7].all() and not unread[:7, :7].any()
    unread = _cnn.unread_positions(_cnn.kernel_case(g, "33x9 k(5,3) s(2,1) p(2,3) d(2,1)", 1, 1))
    assert unread.any(dim=1).sum() == 16 and not unread.all(dim=1).logical_xor(unread.any(dim=1)).any(), "every other row is unread"
