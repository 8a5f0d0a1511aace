"""The gate and GLU kernels and the gate / GLU / FeedForward modules on an MI355X: both launches of every kind against the float64
evaluation of their formulas, saturation, memory safety, views, error codes, the launch census, fallbacks, the reference's
recorded runs (golden ``gates.npz``) and an agent whose actor is built from them.

Worst figures measured on an MI355X over every kernel case (what DESIGN.md "Gates and GLU" quotes): gate forward 5.8e-2 of its
bound (1e-5 relative + 2e-6), gate gradients 2.5e-7 of the largest entry; GLU forward 2.2e-2 of its bound, GLU gradients 1.8e-7;
modules against the recorded runs at most 3.6e-7 of the largest entry."""

from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

import _gates

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE_FWD, GATE_BWD, GLU_FWD, GLU_BWD = "cusrl_gate_fwd", "cusrl_gate_bwd", "cusrl_glu_fwd", "cusrl_glu_bwd"
SYMBOLS = (GATE_FWD, GATE_BWD, GLU_FWD, GLU_BWD)
OPERANDS = ("x", "y", "p", "q", "p2", "q2")
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

    return tuple(_native.launch_counts.get(symbol, 0) for symbol in SYMBOLS)


def _delta(before):
    return tuple(now - then for now, then in zip(_counts(), before))


def _on_device(case):
    return {key: None if value is None else value.to(DEV) for key, value in case.items()}


def _gate_forward_backward(kind, case) -> dict:
    """``out`` and the gradients the kind's backward writes, through the autograd Function: one forward and one backward call.
    Also checked here: the gradient of an operand that enters the output as itself is ``dout``'s bits, and the second addends
    receive the bits of ``dp`` / ``dq``."""
    from cusrl_amd import ops

    leaves = {name: None if case[name] is None else case[name].detach().requires_grad_(True) for name in OPERANDS}
    before = _counts()
    out = ops.GateCombine.apply(kind, *leaves.values())
    present = [name for name in OPERANDS if leaves[name] is not None]
    grads = dict(zip(present, torch.autograd.grad(out, [leaves[name] for name in present], grad_outputs=case["dout"])))
    assert _delta(before) == (1, 1, 0, 0), "one forward and one backward call"
    got = {"out": out.detach()}
    for name in _gates.GRADIENTS[kind]:
        got[name] = grads[name[1:]]
    for name in present:
        if name in ("x", "y") and "d" + name not in _gates.GRADIENTS[kind]:
            assert torch.equal(grads[name], case["dout"].contiguous().view_as(grads[name])), f"d{name} is dout"
    if leaves["p2"] is not None:
        assert torch.equal(grads["p2"], grads["p"])
    if leaves["q2"] is not None:
        assert torch.equal(grads["q2"], grads["q"])
    return got


def _glu_forward_backward(kind, case) -> dict:
    from cusrl_amd import ops

    leaf = case["input"].detach().requires_grad_(True)
    before = _counts()
    out = ops.Glu.apply(kind, leaf)
    (dinput,) = torch.autograd.grad(out, leaf, grad_outputs=case["dout"])
    assert _delta(before) == (0, 0, 1, 1), "one forward and one backward call"
    return {"out": out.detach(), "dinput": dinput}


_WORST: dict[str, float] = {}


def _note(family, errors):
    for name, error in errors.items():
        key = f"{family} {'forward (fraction of 1e-5 rel + 2e-6)' if name == 'out' else 'gradients (of the largest entry)'}"
        _WORST[key] = max(_WORST.get(key, 0.0), error)


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("kind,rows,C", list(itertools.product(_gates.GATE_KINDS, _gates.ROWS, _gates.WIDTHS)))
def test_gate_kernels_match_the_float64_formulas(cusrl, golden, kind, rows, C):
    case = _gates.gate_case(golden("gates"), kind, rows, C)
    device_case = _on_device(case)
    assert all(t is None or t.data_ptr() % 16 == 0 for t in device_case.values())
    got = _gate_forward_backward(kind, device_case)
    _note("gates", _gates.assert_kernel_matches(f"{kind} [{rows}, {C}]", got, _gates.gate_formulas(kind, case, torch.float64)))


@pytest.mark.parametrize("kind,rows,H", list(itertools.product(_gates.GLU_KINDS, _gates.ROWS, _gates.WIDTHS)))
def test_glu_kernels_match_the_float64_formulas(cusrl, golden, kind, rows, H):
    case = _gates.glu_case(golden("gates"), rows, H)
    got = _glu_forward_backward(kind, _on_device(case))
    _note("GLU", _gates.assert_kernel_matches(f"{kind} [{rows}, 2 x {H}]", got, _gates.glu_formulas(kind, case, torch.float64)))


def test_second_addends_with_every_kind(cusrl, golden):
    """``p2`` / ``q2`` with the kinds the modules call without them, and the GRU kinds without."""
    for kind in _gates.GATE_KINDS:
        case = _gates.gate_case(golden("gates"), kind, 257, 50, second=not kind.startswith("gru"))
        got = _gate_forward_backward(kind, _on_device(case))
        _gates.assert_kernel_matches(f"{kind} [257, 50], second addends {'off' if kind.startswith('gru') else 'on'}", got,
                                     _gates.gate_formulas(kind, case, torch.float64))


def test_worst_measured_errors_are_printed():
    """(runs after the parity cases of this module: what DESIGN.md quotes)"""
    for key, error in sorted(_WORST.items()):
        print(f"worst over every kernel case, {key}: {error:.3e}")


def test_saturated_pre_activations_give_finite_outputs_and_zero_gradients(cusrl, golden):
    g = golden("gates")
    for kind in _gates.GATE_KINDS:
        case = _gates.saturated_gate_case(g, kind)
        for shape in ((4, 4), (16, 1)):  # the 16-byte lanes and the 4-byte lanes
            shaped = {name: None if value is None else value.reshape(shape).contiguous() for name, value in case.items()}
            got = _gate_forward_backward(kind, _on_device(shaped))
            _gates.assert_saturated(f"saturated {kind} {shape}", got, _gates.gate_formulas(kind, shaped, torch.float64),
                                    _gates.saturation_masks(kind, shaped))
    for kind in _gates.GLU_KINDS:
        case = _gates.saturated_glu_case(g)
        got = _glu_forward_backward(kind, _on_device(case))
        _gates.assert_saturated(f"saturated {kind}", got, _gates.glu_formulas(kind, case, torch.float64))


# ------------------------------------------------------------------------------------------------ memory safety, raw entry points
def _raw(name):
    from cusrl_amd import _native

    return getattr(_native.lib(), name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


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

    def unchanged(self) -> bool:
        return torch.equal(self.tensor, self.before)

    def ptr(self):
        return self.tensor.data_ptr()


def _ptr(guarded):
    return None if guarded is None else guarded.ptr()


@pytest.mark.parametrize("kind,rows,C", [(kind, rows, C) for kind in _gates.GATE_KINDS for rows, C in ((257, 48), (257, 50), (2049, 4))])
def test_gate_launches_stay_inside_their_operands(cusrl, golden, kind, rows, C):
    """Guard floats behind every operand untouched, inputs unchanged, NaN-filled outputs fully written — and the bits of the
    autograd Function's call."""
    from cusrl_amd import _native

    case = _on_device(_gates.gate_case(golden("gates"), kind, rows, C))
    expected = _gate_forward_backward(kind, case)
    inputs = {name: None if case[name] is None else _Guarded((rows, C), case[name]) for name in (*OPERANDS, "dout")}
    out = _Guarded((rows, C))
    grads = {name: _Guarded((rows, C)) for name in _gates.GRADIENTS[kind]}
    code = _native._CONSTANTS["GATE_" + kind.upper()]
    pointers = [_ptr(inputs[name]) for name in ("x", "y", "p", "p2", "q", "q2")]  # (the C ABI's order)
    assert _raw(GATE_FWD)(code, *pointers, out.ptr(), rows, C, _stream()) == 0
    assert _raw(GATE_BWD)(code, *pointers, inputs["dout"].ptr(), *(_ptr(grads.get(name)) for name in ("dx", "dy", "dp", "dq")), rows, C,
                          _stream()) == 0
    torch.cuda.synchronize()
    for name, guarded in [*inputs.items(), ("out", out), *grads.items()]:
        if guarded is not None:
            assert guarded.guards_intact(), f"{name}: a guard float was written"
    assert all(guarded.unchanged() for guarded in inputs.values() if guarded is not None), "a read-only operand changed"
    assert torch.equal(out.tensor, expected["out"]) and not torch.isnan(out.tensor).any()
    for name, guarded in grads.items():
        assert torch.equal(guarded.tensor, expected[name]) and not torch.isnan(guarded.tensor).any(), name


@pytest.mark.parametrize("kind,rows,H", [(kind, rows, H) for kind in _gates.GLU_KINDS for rows, H in ((257, 48), (257, 50), (2049, 4))])
def test_glu_launches_stay_inside_their_operands(cusrl, golden, kind, rows, H):
    from cusrl_amd import _native

    case = _on_device(_gates.glu_case(golden("gates"), rows, H))
    expected = _glu_forward_backward(kind, case)
    input, dout = _Guarded((rows, 2 * H), case["input"]), _Guarded((rows, H), case["dout"])
    out, dinput = _Guarded((rows, H)), _Guarded((rows, 2 * H))
    code = _native._CONSTANTS["GLU_" + kind.upper()]
    assert _raw(GLU_FWD)(code, input.ptr(), out.ptr(), rows, H, _stream()) == 0
    assert _raw(GLU_BWD)(code, input.ptr(), dout.ptr(), dinput.ptr(), rows, H, _stream()) == 0
    torch.cuda.synchronize()
    assert all(guarded.guards_intact() for guarded in (input, dout, out, dinput)), "a guard float was written"
    assert input.unchanged() and dout.unchanged(), "a read-only operand changed"
    assert torch.equal(out.tensor, expected["out"]) and torch.equal(dinput.tensor, expected["dinput"])
    assert not torch.isnan(out.tensor).any() and not torch.isnan(dinput.tensor).any()


def _offset_view(t):
    """The same values one float off a 16-byte boundary."""
    buffer = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _same(a: dict, b: dict) -> bool:
    return sorted(a) == sorted(b) and all(torch.equal(a[key].reshape(b[key].shape), b[key]) for key in a)


@pytest.mark.parametrize("kind", _gates.GATE_KINDS)
def test_gate_views_give_the_bits_of_the_contiguous_call(cusrl, golden, kind):
    g = golden("gates")
    # an operand one float off the 16-byte boundary at C = 4: the 4-byte lanes, the same bits
    case = _on_device(_gates.gate_case(g, kind, 257, 4))
    aligned = _gate_forward_backward(kind, case)
    for shifted in [name for name in (*OPERANDS, "dout") if case[name] is not None]:
        moved = dict(case)
        moved[shifted] = _offset_view(case[shifted])
        assert _same(_gate_forward_backward(kind, moved), aligned), f"{shifted} as an offset view"
    # a temporal batch [T, B, C] is the [T * B, C] launch
    case = _on_device(_gates.gate_case(g, kind, 15, 6))
    flat = _gate_forward_backward(kind, case)
    temporal = _gate_forward_backward(kind, {name: None if value is None else value.view(5, 3, 6) for name, value in case.items()})
    assert all(value.shape == (5, 3, 6) for value in temporal.values()) and _same(temporal, flat)
    # a transposed (non-contiguous) x and dout are staged
    case = _on_device(_gates.gate_case(g, kind, 48, 257))
    transposed = {name: None if value is None else value.t().contiguous() for name, value in case.items()}  # [257, 48]
    strided = dict(transposed, x=case["x"].t(), dout=case["dout"].t())
    assert not strided["x"].is_contiguous() and not strided["dout"].is_contiguous()
    staged = _gate_forward_backward(kind, strided)
    assert all(value.is_contiguous() for value in staged.values()) and _same(staged, _gate_forward_backward(kind, transposed))


@pytest.mark.parametrize("kind", _gates.GLU_KINDS)
def test_glu_views_give_the_bits_of_the_contiguous_call(cusrl, golden, kind):
    g = golden("gates")
    case = _on_device(_gates.glu_case(g, 257, 4))
    aligned = _glu_forward_backward(kind, case)
    for shifted in ("input", "dout"):
        assert _same(_glu_forward_backward(kind, dict(case, **{shifted: _offset_view(case[shifted])})), aligned), shifted
    case = _on_device(_gates.glu_case(g, 15, 6))
    temporal = _glu_forward_backward(kind, {"input": case["input"].view(5, 3, 12), "dout": case["dout"].view(5, 3, 6)})
    assert temporal["out"].shape == (5, 3, 6) and temporal["dinput"].shape == (5, 3, 12)
    assert _same(temporal, _glu_forward_backward(kind, case))
    case = _on_device(_gates.glu_case(g, 260, 24))  # input [260, 48] and dout [260, 24] with strides (1, 260)
    strided = {name: value.t().contiguous().t() for name, value in case.items()}
    assert not strided["input"].is_contiguous() and not strided["dout"].is_contiguous()
    staged = _glu_forward_backward(kind, strided)
    assert all(value.is_contiguous() for value in staged.values()) and _same(staged, _glu_forward_backward(kind, case))


def test_error_codes(cusrl):
    """Straight through ctypes; none of these calls launches anything."""
    from cusrl_amd import _native

    invalid = _native._CONSTANTS["E_INVALID"]
    tensors = {name: torch.ones(3, 4, device=DEV) for name in (*OPERANDS, "dout")}
    outputs = {name: torch.full((3, 4), 7.0, device=DEV) for name in ("out", "dx", "dy", "dp", "dq", "wide")}
    X, Y, P, Q, P2, Q2, D = (tensors[name].data_ptr() for name in (*OPERANDS, "dout"))
    O, DX, DY, DP, DQ = (outputs[name].data_ptr() for name in ("out", "dx", "dy", "dp", "dq"))
    fwd, bwd, glu_fwd, glu_bwd, s = _raw(GATE_FWD), _raw(GATE_BWD), _raw(GLU_FWD), _raw(GLU_BWD), _stream()
    kinds = {kind: _native._CONSTANTS["GATE_" + kind.upper()] for kind in _gates.GATE_KINDS}
    for kind, code in kinds.items():
        good = (code, X, Y, P, P2, Q, Q2, O, 3, 4)
        bad = [(code, None, Y, P, P2, Q, Q2, O, 3, 4), (code, X, Y, None, P2, Q, Q2, O, 3, 4), (code, X, Y, P, P2, Q, Q2, None, 3, 4),
               (code, X, Y, P, P2, Q, Q2, O, -1, 4), (code, X, Y, P, P2, Q, Q2, O, 3, 0), (code, X, Y, P, P2, Q, Q2, O, 3, -4)]
        if _gates.TAKES_Y[kind]:
            bad.append((code, X, None, P, P2, Q, Q2, O, 3, 4))
        if _gates.TAKES_Q[kind]:
            bad.append((code, X, Y, P, P2, None, Q2, O, 3, 4))  # a q missing for a kind that needs it
        for arguments in bad:
            assert fwd(*arguments, s) == invalid, (kind, arguments)
        assert fwd(*good[:8], 0, 4, s) == 0, "rows == 0 is a successful no-op"
        good = (code, X, Y, P, P2, Q, Q2, D, DX, DY, DP, DQ, 3, 4)
        bad = [(code, X, Y, None, P2, Q, Q2, D, DX, DY, DP, DQ, 3, 4), (code, X, Y, P, P2, Q, Q2, None, DX, DY, DP, DQ, 3, 4),
               (code, X, Y, P, P2, Q, Q2, D, DX, DY, None, DQ, 3, 4), (code, X, Y, P, P2, Q, Q2, D, DX, DY, DP, DQ, -1, 4),
               (code, X, Y, P, P2, Q, Q2, D, DX, DY, DP, DQ, 3, 0)]
        if "dx" in _gates.GRADIENTS[kind]:
            bad += [(code, None, Y, P, P2, Q, Q2, D, DX, DY, DP, DQ, 3, 4), (code, X, Y, P, P2, Q, Q2, D, None, DY, DP, DQ, 3, 4)]
        if "dy" in _gates.GRADIENTS[kind]:
            bad += [(code, X, None, P, P2, Q, Q2, D, DX, DY, DP, DQ, 3, 4), (code, X, Y, P, P2, Q, Q2, D, DX, None, DP, DQ, 3, 4)]
        if "dq" in _gates.GRADIENTS[kind]:
            bad += [(code, X, Y, P, P2, None, Q2, D, DX, DY, DP, DQ, 3, 4), (code, X, Y, P, P2, Q, Q2, D, DX, DY, DP, None, 3, 4)]
        for arguments in bad:
            assert bwd(*arguments, s) == invalid, (kind, arguments)
        assert bwd(*good[:12], 0, 4, s) == 0
    for code in (-1, 6, 99):  # an unknown kind
        assert fwd(code, X, Y, P, P2, Q, Q2, O, 3, 4, s) == invalid and bwd(code, X, Y, P, P2, Q, Q2, D, DX, DY, DP, DQ, 3, 4, s) == invalid
    W = outputs["wide"].data_ptr()  # ([3, 4] read as input [3, 2 x 2])
    for code in (0, 1):
        for arguments in ((code, None, O, 3, 2), (code, X, None, 3, 2), (code, X, O, -1, 2), (code, X, O, 3, 0), (code, X, O, 3, -2)):
            assert glu_fwd(*arguments, s) == invalid, arguments
        for arguments in ((code, None, D, W, 3, 2), (code, X, None, W, 3, 2), (code, X, D, None, 3, 2), (code, X, D, W, -1, 2), (code, X, D, W, 3, 0)):
            assert glu_bwd(*arguments, s) == invalid, arguments
        assert glu_fwd(code, X, O, 0, 2, s) == 0 and glu_bwd(code, X, D, W, 0, 2, s) == 0
    for code in (-1, 2):
        assert glu_fwd(code, X, O, 3, 2, s) == invalid and glu_bwd(code, X, D, W, 3, 2, s) == invalid
    torch.cuda.synchronize()
    assert all(torch.equal(value, torch.full((3, 4), 7.0, device=DEV)) for value in outputs.values()), "a refused call wrote"
    assert invalid < 0


# ------------------------------------------------------------------------------------------------ launch census
# module -> (gate launches, GLU launches) per direction when a gradient is asked for (DESIGN.md "Gates and GLU")
BUDGET = {("gate", "passthrough"): (0, 0), ("gate", "residual"): (0, 0), ("gate", "input"): (1, 0), ("gate", "output"): (1, 0),
          ("gate", "highway"): (1, 0), ("gate", "sigmoid_tanh"): (1, 0), ("gate", "gru"): (2, 0), ("glu", "geglu"): (0, 1),
          ("glu", "swiglu"): (0, 1), ("ff", "geglu"): (0, 1), ("ff", "swiglu"): (0, 1), ("ff", "gelu"): (0, 0)}


@pytest.mark.parametrize("family,name,size", _gates.MODULE_CASES)
def test_module_reproduces_the_reference_on_the_device_within_its_launch_budget(cusrl, golden, family, name, size):
    g = golden("gates")
    prefix = _gates.module_prefix(family, name, size)
    module = _gates.build_module(cusrl, family, name, size)
    module.load_state_dict(_gates.recorded_state(g, prefix), strict=True)
    module.to(DEV)
    inputs, w = _gates.module_inputs(g, family, name, size)
    gates, glus = BUDGET[family, name]
    before = _counts()
    got = _gates.run_module(module, inputs, w, DEV)
    assert _delta(before) == (gates, gates, glus, glus), "forward and backward launches with a gradient asked for"
    _gates.assert_module_matches(prefix + " on the device", got, g, prefix)
    with torch.no_grad():  # without a gradient: the forward launches alone, the same output bits
        before = _counts()
        again = module(*(value.to(DEV) for value in inputs.values()))
        assert _delta(before) == (gates, 0, glus, 0) and torch.equal(again, got["out"])
    before = _counts()  # a forward with a gradient asked for launches no backward until it is asked for
    output = module(*(value.to(DEV).requires_grad_(True) for value in inputs.values()))
    assert _delta(before) == (gates, 0, glus, 0) and torch.equal(output.detach(), got["out"])


# ------------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("form", ["autocast", "float64", "double_differentiable"])
def test_fallbacks_leave_the_kernels_alone(cusrl, golden, form):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable
    from cusrl_amd.ops.gate import _gate_expression, _glu_expression

    g = golden("gates")
    dtype = torch.float64 if form == "float64" else torch.float32

    def evaluate(function, *arguments):
        with torch.autocast("cuda", enabled=form == "autocast"):
            if form == "double_differentiable":
                with double_differentiable():
                    return function(*arguments)
            return function(*arguments)

    def leaves_of(case, names):
        return {name: None if case[name] is None else case[name].to(dtype).requires_grad_(True) for name in names}

    def compare(out, out_ref, leaves):
        assert out.dtype == out_ref.dtype and torch.equal(out, out_ref)
        present = [leaf for leaf in leaves.values() if leaf is not None]
        # (the same kind of backward on both sides: with create_graph torch differentiates gelu / silu through other kernels
        # than its fused backward, and the two differ in the last bit)
        differentiable = form == "double_differentiable"
        grads = torch.autograd.grad(out.float().square().sum(), present, create_graph=differentiable)
        grads_ref = torch.autograd.grad(out_ref.float().square().sum(), present, create_graph=differentiable)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads_ref))
        if form == "double_differentiable":  # a second differentiation goes through torch's own differentiable ops
            (second,) = torch.autograd.grad(sum(grad.square().sum() for grad in grads), present[0])
            assert torch.isfinite(second).all() and second.abs().sum() > 0

    before = _counts()
    for kind in _gates.GATE_KINDS:
        leaves = leaves_of(_on_device(_gates.gate_case(g, kind, 40, 12, second=True)), OPERANDS)
        assert not evaluate(ops.gate_supported, kind, *leaves.values())
        compare(evaluate(ops.gate_combine, kind, *leaves.values()), evaluate(_gate_expression, kind, *leaves.values()), leaves)
    for kind in _gates.GLU_KINDS:
        leaves = leaves_of(_on_device(_gates.glu_case(g, 40, 6)), ("input",))
        assert not evaluate(ops.glu_supported, leaves["input"])
        compare(evaluate(ops.glu, kind, leaves["input"]), evaluate(_glu_expression, kind, leaves["input"], -1), leaves)
    assert _delta(before) == (0, 0, 0, 0)
    for kind in _gates.GLU_KINDS:  # a split along another dimension: torch's expression in every form, plain fp32 included
        leaf = _on_device(_gates.glu_case(g, 40, 6))["input"].requires_grad_(True)
        assert not ops.glu_supported(leaf, 0) and ops.glu_supported(leaf, 1) and ops.glu_supported(leaf, -1)
        out, out_ref = ops.glu(kind, leaf, dim=0), _glu_expression(kind, leaf, 0)
        assert out.shape == (20, 12) and torch.equal(out, out_ref)
        assert torch.equal(*(torch.autograd.grad(o.square().sum(), leaf)[0] for o in (out, out_ref)))
    assert _delta(before) == (0, 0, 0, 0)
    if form == "double_differentiable":  # inside the context a pass nobody differentiates launches
        case = _on_device(_gates.gate_case(g, "highway", 40, 12))
        with double_differentiable(), torch.no_grad():
            ops.gate_combine("highway", case["x"], case["y"], case["p"])
            ops.glu("swiglu", case["x"])
        assert _delta(before) == (1, 0, 1, 0)


# ------------------------------------------------------------------------------------------------ an agent
def test_agent_with_a_gated_glu_backbone_trains(cusrl):
    """``Mlp -> FeedForward(SwiGlu)`` merged by a ``HighwayGate`` as the actor's backbone in the eager ``ppo`` preset: 8 envs,
    4 steps per update, 2 epochs x 2 minibatches, 2 iterations."""

    class GatedBackbone(cusrl.Module):
        batch_invariant = False  # (library GEMMs: their summation order depends on the row count)

        def __init__(self, input_dim, hidden_dim=16):
            super().__init__(input_dim, hidden_dim)
            self.mlp = cusrl.Mlp(input_dim, [hidden_dim], ends_with_activation=True)
            self.feedforward = cusrl.FeedForward(hidden_dim, 32, cusrl.SwiGlu)
            self.gate = cusrl.HighwayGate(hidden_dim)

        def forward(self, input, **kwargs):
            latent = self.mlp(input)
            return self.gate(latent, self.feedforward(latent))

    class Census(cusrl.Hook):
        def __init__(self):
            super().__init__()
            self.marks = []

        def pre_update(self, buffer):
            self.marks.append(_counts())

        def post_update(self):
            self.marks.append(_counts())

    cusrl.set_global_seed(11)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=10, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=4, sampler_epochs=2, sampler_mini_batches=2).to_underlying()
    factory.actor_factory.backbone_factory = lambda input_dim, output_dim=None: GatedBackbone(input_dim)
    census = Census()
    factory.register_hook(census)
    trainer = cusrl.Trainer(env, factory, num_iterations=2, verbose=False)
    agent = trainer.agent
    assert isinstance(agent.actor.backbone, GatedBackbone)
    gate_parameters = [name for name, _ in agent.named_parameters() if ".gate.gate_linear." in name]
    assert len(gate_parameters) == 2, gate_parameters
    initial = {name: param.detach().clone() for name, param in agent.named_parameters()}
    start = _counts()
    trainer.run_training_loop()
    torch.cuda.synchronize()
    assert len(census.marks) == 4  # pre_update, post_update, twice
    marks = [start, *census.marks]
    rollouts = [tuple(b - a for a, b in zip(marks[i], marks[i + 1])) for i in (0, 2)]
    updates = [tuple(b - a for a, b in zip(marks[i], marks[i + 1])) for i in (1, 3)]
    print(f"(gate fwd, gate bwd, glu fwd, glu bwd) launches: rollouts {rollouts}, updates {updates}")
    for gate_fwd, _, glu_fwd, _ in rollouts:
        assert gate_fwd >= 4 and glu_fwd >= 4, "one launch of each per act step"
    for gate_fwd, gate_bwd, glu_fwd, glu_bwd in updates:
        assert min(gate_fwd, gate_bwd, glu_fwd, glu_bwd) >= 2 * 2, "one launch of each per minibatch step and direction"
    for key in ("Agent/value_loss", "Agent/surrogate_loss", "Agent/kl_divergence"):
        if key in trainer.last_info:
            assert np.isfinite(trainer.last_info[key]), key
    assert np.isfinite(trainer.last_info["Agent/value_loss"])
    for name, param in agent.named_parameters():
        assert torch.isfinite(param).all(), name
        if param.requires_grad:
            assert not torch.equal(param, initial[name]), f"{name} did not change"
