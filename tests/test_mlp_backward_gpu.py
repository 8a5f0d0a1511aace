"""The MLP backward kernels on an MI355X — ``cusrl_narrow_linear_bwd`` with its finalize, ``cusrl_narrow_linear_fwd``,
``cusrl_input_layer_bwd`` with its row sum, ``cusrl_relu_bwd_colsum`` with its finalizes — at every instantiation and edge of
the tables of tests/_mlp_backward.py.

Lattice cases are asserted with ``torch.equal`` against the float64 result cast to fp32 (tests/test_mlp_backward.py shows on
the CPU that any correct evaluation gives those bits): every element of every row counted exactly once, in the right slot.
Float cases are held to the bounds the project already holds these kernels to.  The library's own partial counts must equal
the tables' expectations, so a changed default block size fails here instead of un-covering an edge.  The guard-band tests call
the raw C entry points with buffers of exactly the documented sizes."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _mlp_backward as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64  # floats on either side of an operand (256 bytes: the operand keeps its 16-byte alignment)
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from cusrl_amd import ops as _ops

    return _ops


@pytest.fixture
def option(ops):
    """``option(key, value)``: ``cusrl_set_option`` for the duration of the test; the value read beforehand comes back in the
    teardown, also when the test fails (tests/test_hip_kernels.py::test_options_are_validated_and_readable shows the calls)."""
    from cusrl_amd import _native

    before = {}

    def set_(key, value):
        before.setdefault(key, _native.get_option(key))
        _native.set_option(key, value)
        assert _native.get_option(key) == value

    yield set_
    for key, value in before.items():
        _native.set_option(key, value)


def _lib():
    from cusrl_amd import _native

    return _native.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _on_device(tensors: dict) -> dict:
    return {name: None if value is None else value.to(DEV) for name, value in tensors.items()}


def _lattice(cases):
    return [case for case in cases if M.is_lattice(case)]


def _float(cases):
    return [case for case in cases if not M.is_lattice(case)]


def _host(tensors: dict) -> dict:
    return {name: value.cpu() for name, value in tensors.items()}


# ------------------------------------------------------------------------------------------------ narrow backward
def _narrow_outputs(ops, case, data, **how) -> dict:
    """dx, dW, db, the column sums and the whole ``packed`` row of one call through ``ops.narrow_linear_backward``."""
    K, O = case.K, case.O
    dx, dW, db, colsum = ops.narrow_linear_backward(data["g"], data["x"], data["w"], relu_input=case.relu_input, **how)
    packed = dW._base
    assert packed is not None and packed.shape == (M.narrow_width(K, O),), "dW is a window of the packed row"
    assert dW.shape == (O, K) and db.shape == (O,) and (colsum is None) == (not case.relu_input)
    if colsum is not None:
        assert colsum.data_ptr() == packed[O * K:].data_ptr() and colsum.shape == (K,)
    return {"dx": dx, "dW": dW, "db": db, "colsum": packed[O * K:(O + 1) * K], "pad": packed[(O + 1) * K + O:]}


@pytest.mark.parametrize("case", _lattice(M.NARROW_CASES), ids=M.ident)
def test_narrow_backward_counts_every_row_once(ops, option, case):
    option("head_rows", case.head_rows)
    assert _lib().cusrl_narrow_linear_num_partials(case.rows) == case.partials, "the table's partial count is the library's"
    assert ops.narrow_linear_supported(case.K, case.O)
    data, want = _on_device(M.inputs(case)), _on_device(M.expected(case))
    got = _narrow_outputs(ops, case, data)
    assert got["dx"].shape == (case.rows, case.K)
    for name in ("dx", "dW", "db", "colsum"):  # (relu_input off: the expected column sums are zeros — the slice stays empty)
        assert torch.equal(got[name], want[name]), f"{case.name}: {name} ({case.edge})"
    assert not got["pad"].any(), "the padding behind db is zero"
    again = _narrow_outputs(ops, case, data, need_input_grad=False)
    assert again["dx"] is None
    for name in ("dW", "db", "colsum"):
        assert torch.equal(again[name], want[name]), f"{case.name}: {name} without grad_input"


@pytest.mark.parametrize("case", _float(M.NARROW_CASES), ids=M.ident)
def test_narrow_backward_float(ops, option, case):
    option("head_rows", case.head_rows)
    assert _lib().cusrl_narrow_linear_num_partials(case.rows) == case.partials
    data = _on_device(M.inputs(case))
    got = _narrow_outputs(ops, case, data)
    M.check_float(case, _host({name: got[name] for name in ("dx", "dW", "db", "colsum")}))
    again = _narrow_outputs(ops, case, data)
    assert all(torch.equal(again[name], got[name]) for name in got), "two launches, the same bits"


# ------------------------------------------------------------------------------------------------ row dot
@pytest.mark.parametrize("case", _lattice(M.ROW_DOT_CASES), ids=M.ident)
def test_row_dot_forward_lattice(ops, case):
    data, want = _on_device(M.inputs(case)), _on_device(M.expected(case))
    assert ops.narrow_linear_forward_supported(data["x"], data["w"])
    out = ops.narrow_linear_forward(data["x"], data["w"], data["b"])
    assert out.shape == (case.rows, 1) and torch.equal(out, want["out"]), f"{case.name} ({case.edge})"


@pytest.mark.parametrize("case", _float(M.ROW_DOT_CASES), ids=M.ident)
def test_row_dot_forward_float(ops, case):
    data = _on_device(M.inputs(case))
    out = ops.narrow_linear_forward(data["x"], data["w"], data["b"])
    M.check_float(case, {"out": out.cpu()})
    assert torch.equal(ops.narrow_linear_forward(data["x"], data["w"], data["b"]), out), "two launches, the same bits"


# ------------------------------------------------------------------------------------------------ input layer
@pytest.mark.parametrize("case", _lattice(M.INPUT_CASES), ids=M.ident)
def test_input_layer_backward_lattice(ops, case):
    assert _lib().cusrl_input_layer_row_blocks(case.rows, case.H) == case.partials, "the table's partial count is the library's"
    data, want = _on_device(M.inputs(case)), _on_device(M.expected(case))
    assert ops.input_layer_supported(data["g"], data["y"], data["x"], torch.empty(case.H, case.K, device=DEV))
    dW, db = ops.input_layer_backward(data["g"], data["y"], data["x"])
    assert dW.shape == (case.H, case.K) and db.shape == (case.H,)
    assert torch.equal(dW, want["dW"]) and torch.equal(db, want["db"]), f"{case.name} ({case.edge})"


@pytest.mark.parametrize("case", _float(M.INPUT_CASES), ids=M.ident)
def test_input_layer_backward_float(ops, case, gradient_parity):
    assert _lib().cusrl_input_layer_row_blocks(case.rows, case.H) == case.partials
    data = _on_device(M.inputs(case))
    dW, db = ops.input_layer_backward(data["g"], data["y"], data["x"])
    gradient_parity(f"mlp_backward.input_layer.dW[{case.name}]", dW.cpu().numpy(), M.reference(case)["dW"].numpy(), M.INPUT_DW_BOUND)
    M.check_float(case, {"db": db.cpu()})
    again = ops.input_layer_backward(data["g"], data["y"], data["x"])
    assert torch.equal(again[0], dW) and torch.equal(again[1], db), "two launches, the same bits"


# ------------------------------------------------------------------------------------------------ ReLU backward + column sums
def _colsum_outputs(ops, case, data, defer=False):
    grad_in, colsum = ops.relu_backward_bias(data["g"], data["y"], defer=defer)
    if not case.mask:
        assert grad_in is data["g"]
    if defer and case.chunked:
        assert isinstance(colsum, ops.DeferredColumns) and (colsum.splits, colsum.row_stride, colsum.column, colsum.numel) == (
            case.partials, case.H, 0, case.H)
        colsum = colsum.materialize()
    assert colsum.shape == (case.H,)
    return {"grad_in": grad_in, "colsum": colsum}


@pytest.mark.parametrize("case", _lattice(M.COLSUM_CASES), ids=M.ident)
def test_relu_backward_bias_counts_every_row_once(ops, option, case):
    option("colsum_rows", case.colsum_rows)
    assert _lib().cusrl_colsum_num_partials(case.rows, case.H) == case.partials, "the table's partial count is the library's"
    data, want = _on_device(M.inputs(case)), _on_device(M.expected(case))
    for defer in (False, True):  # (a row-wise width has no deferred form: the same finalized sums)
        got = _colsum_outputs(ops, case, data, defer)
        for name in ("grad_in", "colsum"):
            assert torch.equal(got[name], want[name]), f"{case.name}: {name}, defer={defer} ({case.edge})"


@pytest.mark.parametrize("case", _float(M.COLSUM_CASES), ids=M.ident)
def test_relu_backward_bias_float(ops, option, case):
    option("colsum_rows", case.colsum_rows)
    assert _lib().cusrl_colsum_num_partials(case.rows, case.H) == case.partials
    data = _on_device(M.inputs(case))
    got = _colsum_outputs(ops, case, data)
    assert torch.equal(got["grad_in"].double().cpu(), M.reference(case)["grad_in"]), "the mask is exact"
    M.check_float(case, {"colsum": got["colsum"].cpu()})
    again = _colsum_outputs(ops, case, data)
    assert torch.equal(again["grad_in"], got["grad_in"]) and torch.equal(again["colsum"], got["colsum"]), "two launches, the same bits"
    if case.chunked:
        M.check_float(case, {"colsum": _colsum_outputs(ops, case, data, defer=True)["colsum"].cpu()})


# ------------------------------------------------------------------------------------------------ deferred outputs
def _find(cases, **fields):
    return next(case for case in cases if all(getattr(case, name) == value for name, value in fields.items()))


# few partial rows (the assembly's per-element path: at most 16) and many (its cooperative path), on either side of 16 / 17
DEFERRED_NARROW = [_find(M.NARROW_LATTICE, K=128, O=12, relu_input=True), _find(M.NARROW_LATTICE, K=32, O=9, relu_input=False),
                   *(case for case in M.NARROW_FINALIZE if case.partials in (1, 16, 17, 65, 128))]
DEFERRED_COLSUM = [_find(M.COLSUM_LATTICE, H=256, rows=257, colsum_rows=0, mask=True), _find(M.COLSUM_LATTICE, H=8, rows=1025, colsum_rows=4, mask=False),
                   *(case for case in M.COLSUM_LATTICE if "finalize over" in case.edge and case.mask and case.partials in (1, 16, 17, 65, 128))]


@pytest.mark.parametrize("case", DEFERRED_NARROW, ids=M.ident)
def test_deferred_narrow_windows_assemble_to_the_packed_bits(ops, option, case):
    option("head_rows", case.head_rows)
    K, O = case.K, case.O
    data, want = _on_device(M.inputs(case)), _on_device(M.expected(case))
    packed = _narrow_outputs(ops, case, data)
    dx, dW, db, colsum = ops.narrow_linear_backward(data["g"], data["x"], data["w"], relu_input=case.relu_input, defer=True)
    assert torch.equal(dx, want["dx"]) and (colsum is None) == (not case.relu_input)
    windows = [("dW", dW, 0, O * K), ("db", db, (O + 1) * K, O)] + ([("colsum", colsum, O * K, K)] if case.relu_input else [])
    flat = torch.full((O * K + O + K + 5,), float("nan"), device=DEV)
    pieces, offset = [], 0
    for name, window, column, numel in windows:
        assert isinstance(window, ops.DeferredColumns)
        assert (window.splits, window.row_stride, window.column, window.numel) == (case.partials, M.narrow_width(K, O), column, numel)
        pieces.append((window, offset, numel, 0))
        offset += numel
    pieces.append((None, offset, flat.numel() - offset, 0))
    ops.assemble_gradients(pieces, flat)
    offset = 0
    for name, window, _, numel in windows:
        assembled = flat[offset:offset + numel]
        assert torch.equal(assembled, packed[name].reshape(-1)) and torch.equal(assembled, want[name].reshape(-1)), f"{case.name}: {name}"
        assert torch.equal(window.materialize(), assembled), f"{case.name}: {name} materialized"
        offset += numel
    assert not flat[offset:].any()


@pytest.mark.parametrize("case", DEFERRED_COLSUM, ids=M.ident)
def test_deferred_column_sums_assemble_to_the_finalized_bits(ops, option, case):
    option("colsum_rows", case.colsum_rows)
    data, want = _on_device(M.inputs(case)), _on_device(M.expected(case))
    finalized = _colsum_outputs(ops, case, data)
    grad_in, window = ops.relu_backward_bias(data["g"], data["y"], defer=True)
    assert isinstance(window, ops.DeferredColumns) and window.splits == case.partials and torch.equal(grad_in, want["grad_in"])
    flat = torch.full((3 + case.H,), float("nan"), device=DEV)
    ops.assemble_gradients([(None, 0, 3, 0), (window, 3, case.H, 0)], flat)
    assert not flat[:3].any() and torch.equal(flat[3:], finalized["colsum"]) and torch.equal(flat[3:], want["colsum"])
    assert torch.equal(window.materialize(), finalized["colsum"])


# ------------------------------------------------------------------------------------------------ raw entry points
class _Guarded:
    """A tensor inside a buffer with ``GUARD`` sentinel floats on either side; ``shift``: one float off the 16-byte boundary.
    ``values`` None: an output, filled with NaN."""

    def __init__(self, shape, values=None, shift=False):
        numel, start = int(np.prod(shape)), GUARD + int(shift)
        self.buffer = torch.full((start + numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.front, self.back = self.buffer[:start], self.buffer[start + numel:]
        self.tensor = self.buffer[start:start + numel].view(shape)
        self.tensor.copy_(values) if values is not None else self.tensor.fill_(float("nan"))
        self.before = self.tensor.clone()
        self.is_output = values is None
        assert self.tensor.data_ptr() % 16 == (4 if shift else 0)

    def guards_intact(self) -> bool:
        return bool((self.front == SENTINEL).all() and (self.back == SENTINEL).all())

    def unchanged(self) -> bool:
        return torch.equal(self.tensor, self.before) or (self.is_output and bool(torch.isnan(self.tensor).all()))

    def written(self) -> bool:
        return not bool(torch.isnan(self.tensor).any())

    def ptr(self):
        return self.tensor.data_ptr()


def _buffers(layout: dict, shifted: str | None) -> dict:
    """``layout``: name -> (shape, values or None for an output) or None for an absent operand."""
    return {name: None if spec is None else _Guarded(spec[0], spec[1], shift=name == shifted) for name, spec in layout.items()}


def _ptrs(buffers: dict, *names):
    return [None if buffers[name] is None else buffers[name].ptr() for name in names]


def _assert_inside(buffers: dict, rc: int, what: str):
    """After a successful launch: no guard float changed, no input changed, every output element written."""
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: status {rc}"
    for name, guarded in buffers.items():
        if guarded is None:
            continue
        assert guarded.guards_intact(), f"{what}: a guard float of {name} was written"
        if guarded.is_output:
            assert guarded.written(), f"{what}: {name} has elements nobody wrote"
        else:
            assert guarded.unchanged(), f"{what}: the read-only operand {name} changed"


def _assert_refused(buffers: dict, rc: int, what: str):
    """A call refused for an unaligned pointer: CUSRL_E_UNSUPPORTED, and nothing written anywhere."""
    torch.cuda.synchronize()
    assert rc == M.UNSUPPORTED, f"{what}: status {rc}, expected CUSRL_E_UNSUPPORTED"
    for name, guarded in buffers.items():
        assert guarded is None or (guarded.guards_intact() and guarded.unchanged()), f"{what}: the refused call wrote to {name}"


def _narrow_raw(case, shifted=None, with_grad_input=True):
    data = M.inputs(case)
    rows, K, O, width = case.rows, case.K, case.O, M.narrow_width(case.K, case.O)
    buffers = _buffers({"g": ((rows, O), data["g"]), "x": ((rows, K), data["x"]), "w": ((O, K), data["w"]),
                        "dx": ((rows, K), None) if with_grad_input else None, "partials": ((case.partials, width), None),
                        "packed": ((width,), None)}, shifted)
    rc = _lib().cusrl_narrow_linear_bwd(*_ptrs(buffers, "g", "x", "w", "dx", "partials", "packed"), rows, K, O, int(case.relu_input), _stream())
    return rc, buffers


def _assert_narrow_exact(case, buffers):
    K, O = case.K, case.O
    want = _on_device(M.expected(case))
    packed, partials = buffers["packed"].tensor, buffers["partials"].tensor
    if buffers["dx"] is not None:
        assert torch.equal(buffers["dx"].tensor, want["dx"])
    assert torch.equal(packed[:O * K].view(O, K), want["dW"]) and torch.equal(packed[O * K:(O + 1) * K], want["colsum"])
    assert torch.equal(packed[(O + 1) * K:(O + 1) * K + O], want["db"]) and not packed[(O + 1) * K + O:].any()
    assert torch.equal(partials.double().sum(0), packed.double()), "the partial rows sum to the packed row"


@pytest.mark.parametrize("case", M.GUARD_NARROW, ids=M.ident)
def test_narrow_backward_stays_inside_its_operands(ops, option, case):
    """Partial rows and ``packed`` of exactly ``P x ((O + 1) K + 16)`` and ``(O + 1) K + 16`` floats; with and without ``grad_input``."""
    option("head_rows", 0)
    assert case.partials > 1 and case.rows % M.HEAD_ROWS != 0
    for with_grad_input in (True, False):
        rc, buffers = _narrow_raw(case, with_grad_input=with_grad_input)
        _assert_inside(buffers, rc, f"{case.name}, grad_input {with_grad_input}")
        _assert_narrow_exact(case, buffers)


def _colsum_raw(case, shifted=None):
    data = M.inputs(case)
    rows, H = case.rows, case.H
    buffers = _buffers({"g": ((rows, H), data["g"]), "y": ((rows, H), data["y"]) if case.mask else None,
                        "grad_in": ((rows, H), None) if case.mask else None, "partials": ((case.partials, H), None), "colsum": ((H,), None)}, shifted)
    rc = _lib().cusrl_relu_bwd_colsum(*_ptrs(buffers, "g", "y", "grad_in", "partials", "colsum"), rows, H, _stream())
    return rc, buffers


def _assert_colsum_exact(case, buffers):
    want = _on_device(M.expected(case))
    if case.mask:
        assert torch.equal(buffers["grad_in"].tensor, want["grad_in"])
    assert torch.equal(buffers["colsum"].tensor, want["colsum"])


@pytest.mark.parametrize("case", M.GUARD_COLSUM, ids=M.ident)
def test_relu_backward_bias_stays_inside_its_operands(ops, option, case):
    """Partial rows and ``colsum`` of exactly ``P x H`` and ``H`` floats."""
    option("colsum_rows", 0)
    assert case.partials == (5 if case.H == 64 else 2 if case.H == 8 else 1)
    rc, buffers = _colsum_raw(case)
    _assert_inside(buffers, rc, case.name)
    _assert_colsum_exact(case, buffers)
    assert torch.equal(buffers["partials"].tensor.double().sum(0), buffers["colsum"].tensor.double())


def _input_raw(case, shifted=None):
    data = M.inputs(case)
    rows, K, H, width = case.rows, case.K, case.H, M.input_layer_width(case.K, case.H)
    buffers = _buffers({"g": ((rows, H), data["g"]), "y": ((rows, H), data["y"]) if case.mask else None, "x": ((rows, K), data["x"]),
                        "partials": ((case.partials, width), None), "grads": ((width,), None)}, shifted)
    rc = _lib().cusrl_input_layer_bwd(*_ptrs(buffers, "g", "y", "x"), rows, K, H, *_ptrs(buffers, "partials", "grads"), _stream())
    return rc, buffers


@pytest.mark.parametrize("case", M.GUARD_INPUT, ids=M.ident)
def test_input_layer_backward_stays_inside_its_operands(ops, case):
    """Partial rows and the gradient row of exactly ``blocks x (H K + H)`` and ``H K + H`` floats."""
    assert case.partials == 3
    rc, buffers = _input_raw(case)
    _assert_inside(buffers, rc, case.name)
    want, grads = _on_device(M.expected(case)), buffers["grads"].tensor
    assert torch.equal(grads[:case.H * case.K].view(case.H, case.K), want["dW"]) and torch.equal(grads[case.H * case.K:], want["db"])
    assert torch.equal(buffers["partials"].tensor.double().sum(0), grads.double())


def _row_dot_raw(case, shifted=None):
    data = M.inputs(case)
    buffers = _buffers({"x": ((case.rows, case.K), data["x"]), "w": ((1, case.K), data["w"]), "b": ((1,), data["b"]) if case.bias else None,
                        "out": ((case.rows,), None)}, shifted)
    rc = _lib().cusrl_narrow_linear_fwd(*_ptrs(buffers, "x", "w", "b", "out"), case.rows, case.K, 1, _stream())
    return rc, buffers


@pytest.mark.parametrize("case", M.GUARD_ROW_DOT, ids=M.ident)
def test_row_dot_forward_stays_inside_its_operands(ops, case):
    """An output of exactly ``rows`` floats."""
    rc, buffers = _row_dot_raw(case)
    _assert_inside(buffers, rc, case.name)
    assert torch.equal(buffers["out"].tensor, _on_device(M.expected(case))["out"].view(-1))


# ------------------------------------------------------------------------------------------------ unaligned operands
@pytest.mark.parametrize("colsum_rows", [0, 4])
@pytest.mark.parametrize("case", [M.GUARD_COLSUM[0], M.GUARD_COLSUM[1], M.GUARD_COLSUM[4]], ids=M.ident)
def test_relu_backward_bias_takes_unaligned_operands_in_its_scalar_forms(ops, option, case, colsum_rows):
    """``grad``, ``output`` or ``grad_in`` one float off: the row-wise kernel over a chunked width; ``colsum`` one float off: the
    scalar finalize over the chunked partial rows (5 and 65 of them at [257, 64]).  The lattice result, exactly, and nothing
    written outside."""
    option("colsum_rows", colsum_rows)
    case = case._replace(colsum_rows=colsum_rows)
    assert case.chunked and _lib().cusrl_colsum_num_partials(case.rows, case.H) == case.partials
    for shifted in ("g", "y", "grad_in", "colsum") if case.mask else ("g", "colsum"):
        rc, buffers = _colsum_raw(case, shifted)
        torch.cuda.synchronize()
        assert rc == 0, shifted
        for name, guarded in buffers.items():
            if guarded is not None:
                assert guarded.guards_intact(), f"{shifted} shifted: a guard float of {name} was written"
                assert guarded.is_output or guarded.unchanged(), f"{shifted} shifted: {name} changed"
        assert buffers["colsum"].written() and (not case.mask or buffers["grad_in"].written())
        _assert_colsum_exact(case, buffers)


def test_unaligned_operands_of_the_vector_kernels_are_refused(ops, option):
    """Each pointer the entry checks of the narrow backward, the row dot and the input layer name, one float off:
    CUSRL_E_UNSUPPORTED and not a byte written.  A ``grad_out`` one float off is only refused where its rows are read as 16-byte
    chunks (``O % 4 == 0``); at O = 9 the call goes through and is exact."""
    option("head_rows", 0)
    wide, odd = M.GUARD_NARROW[1], M.GUARD_NARROW[0]
    assert wide.O % 4 == 0 and odd.O % 4 != 0
    for shifted in ("g", "x", "w", "dx", "partials", "packed"):
        rc, buffers = _narrow_raw(wide, shifted)
        _assert_refused(buffers, rc, f"narrow backward, {shifted} shifted")
    for shifted in ("x", "w", "dx", "partials", "packed"):
        rc, buffers = _narrow_raw(odd, shifted)
        _assert_refused(buffers, rc, f"narrow backward at O = 9, {shifted} shifted")
    rc, buffers = _narrow_raw(odd, "g")
    _assert_inside(buffers, rc, "narrow backward at O = 9, grad_out shifted")
    _assert_narrow_exact(odd, buffers)
    for case in M.GUARD_ROW_DOT:
        for shifted in ("x", "w"):
            rc, buffers = _row_dot_raw(case, shifted)
            _assert_refused(buffers, rc, f"row dot {case.name}, {shifted} shifted")
    for case in M.GUARD_INPUT:
        for shifted in ("g", "y", "x", "partials", "grads") if case.mask else ("g", "x", "partials", "grads"):
            rc, buffers = _input_raw(case, shifted)
            _assert_refused(buffers, rc, f"input layer {case.name}, {shifted} shifted")
