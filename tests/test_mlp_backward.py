"""What tests/test_mlp_backward_gpu.py relies on, shown without a GPU: the float64 restatements of the four MLP backward
operations (tests/_mlp_backward.py) are float64 ``torch.autograd``; every lattice case is exact — its expected values are
integers below 2^24 and an fp32 evaluation in another, shuffled order gives the same bits, so ``torch.equal`` on the device is a
fair assertion for any correct kernel; correct fp32 arithmetic stays inside the float bounds; and the case tables cover the
instantiations and edges they claim, computed from the restated kernel constants."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mlp_backward as M

LATTICE = [case for case in M.ALL_CASES if M.is_lattice(case)]
FLOAT = [case for case in M.ALL_CASES if not M.is_lattice(case)]


# ------------------------------------------------------------------------------------------------ references are autograd
def _draws(values, seed):
    draw = M.lattice if values == "lattice" else M.normal
    return lambda *shape: draw(shape, seed + len(shape) * 7 + sum(shape)).double()


def _close(got, want, values):
    if values == "lattice":
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("values", ["lattice", "normal"])
@pytest.mark.parametrize("rows,K,O", [(1, 32, 1), (37, 64, 9), (197, 128, 16)])
@pytest.mark.parametrize("relu_input", [False, True])
def test_narrow_backward_is_float64_autograd(values, rows, K, O, relu_input):
    draw = _draws(values, rows + K + O)
    pre, w, b, g = draw(rows, K).requires_grad_(True), draw(O, K).requires_grad_(True), draw(O).requires_grad_(True), draw(rows, O)
    x = torch.relu(pre) if relu_input else pre
    F.linear(x, w, b).backward(g)
    dx, dW, db, colsum = M.narrow_backward(g, x.detach(), w.detach(), relu_input)
    _close(dx, pre.grad, values), _close(dW, w.grad, values), _close(db, b.grad, values)
    _close(colsum, pre.grad.sum(0) if relu_input else torch.zeros(K, dtype=torch.float64), values)
    if relu_input and values == "lattice":
        assert bool((x == 0).any()) and bool((pre.grad[x.detach() == 0] == 0).all())  # the ReLU passes nothing at 0


@pytest.mark.parametrize("values", ["lattice", "normal"])
@pytest.mark.parametrize("rows,K", [(1, 32), (33, 1024)])
@pytest.mark.parametrize("bias", [True, False])
def test_row_dot_is_float64_linear(values, rows, K, bias):
    draw = _draws(values, rows + K)
    x, w, b = draw(rows, K), draw(1, K), draw(1) if bias else None
    _close(M.row_dot(x, w, b), F.linear(x, w, b), values)


@pytest.mark.parametrize("values", ["lattice", "normal"])
@pytest.mark.parametrize("rows,K,H", [(1, 4, 64), (37, 60, 128)])
@pytest.mark.parametrize("mask", [True, False])
def test_input_layer_is_float64_autograd(values, rows, K, H, mask):
    draw = _draws(values, rows + K + H)
    x, w, b, g = draw(rows, K), draw(H, K).requires_grad_(True), draw(H).requires_grad_(True), draw(rows, H)
    y = F.linear(x, w, b)
    if mask:
        y = torch.relu(y)
    y.backward(g)
    dW, db = M.input_layer(g, y.detach() if mask else None, x)
    _close(dW, w.grad, values), _close(db, b.grad, values)


@pytest.mark.parametrize("values", ["lattice", "normal"])
@pytest.mark.parametrize("rows,H", [(1, 1), (65, 12), (257, 64)])
@pytest.mark.parametrize("mask", [True, False])
def test_relu_colsum_is_float64_autograd(values, rows, H, mask):
    draw = _draws(values, rows + H)
    pre, b, g = draw(rows, H).requires_grad_(True), draw(H).requires_grad_(True), draw(rows, H)
    y = pre + b
    if mask:
        y = torch.relu(y)
    y.backward(g)
    grad_in, colsum = M.relu_colsum(g, y.detach() if mask else None)
    _close(grad_in, pre.grad, values), _close(colsum, b.grad, values)


# ------------------------------------------------------------------------------------------------ fp32 restatements
def _f32_outputs(case, shuffled: bool) -> dict:
    """The case's outputs in numpy float32: every product and partial sum rounded to fp32.  ``shuffled``: the rows enter the sums
    in a random order and the features / outputs in reversed order — another summation order than the first evaluation's."""
    data = {name: None if value is None else value.numpy() for name, value in M.inputs(case).items()}
    rng = np.random.default_rng(case.seed)
    order = rng.permutation(case.rows) if shuffled else np.arange(case.rows)
    flip = (lambda a, axis: np.flip(a, axis)) if shuffled else (lambda a, axis: a)
    f = np.float32
    if isinstance(case, M.Narrow):
        g, x, w = data["g"], data["x"], data["w"]
        dx = (flip(g, 1) @ flip(w, 0)).astype(f)
        if case.relu_input:
            dx = np.where(x > 0, dx, f(0))
        return {"dx": dx, "dW": (g[order].T @ x[order]).astype(f), "db": g[order].sum(0, dtype=f),
                "colsum": dx[order].sum(0, dtype=f) if case.relu_input else np.zeros(case.K, f)}
    if isinstance(case, M.RowDot):
        out = (flip(data["x"], 1) @ flip(data["w"], 1).T).astype(f)
        return {"out": out if data["b"] is None else out + data["b"]}
    masked = data["g"] if data["y"] is None else np.where(data["y"] > 0, data["g"], f(0))
    if isinstance(case, M.InputLayer):
        return {"dW": (masked[order].T @ data["x"][order]).astype(f), "db": masked[order].sum(0, dtype=f)}
    return {"grad_in": masked, "colsum": masked[order].sum(0, dtype=f)}


@pytest.mark.parametrize("case", LATTICE, ids=M.ident)
def test_lattice_cases_are_exact_in_any_order(case):
    """The float64 results are integers below 2^24, and two fp32 evaluations in different orders give their bits: what makes
    ``torch.equal`` a fair assertion on the device."""
    assert case.rows <= M.MAX_ROWS
    for value in M.inputs(case).values():
        if value is not None:
            assert value.dtype == torch.float32 and bool((value == value.round()).all()) and float(value.abs().max()) <= 2
    want = M.expected(case)
    for name, value in M.reference(case).items():
        assert bool((value == value.round()).all()) and float(value.abs().max()) <= 4 * max(case.rows, 1024) + 2 < 2**24, name
        assert torch.equal(want[name].double(), value), name
    for shuffled in (False, True):
        got = _f32_outputs(case, shuffled)
        assert sorted(got) == sorted(want)
        for name, value in got.items():
            assert value.dtype == np.float32 and np.array_equal(value, want[name].numpy()), (name, shuffled)
    if getattr(case, "mask", False) or getattr(case, "relu_input", False):  # exact zeros where ``> 0`` is decided
        gate = M.inputs(case)["x" if isinstance(case, M.Narrow) else "y"]
        assert bool((gate >= 0).all()) and (gate.numel() < 64 or (bool((gate == 0).any()) and bool((gate > 0).any())))


def test_a_dropped_or_doubled_row_changes_a_lattice_result():
    """What the exact comparison buys: leaving any ONE row out of the sums, or counting it twice, changes an expected tensor
    by a non-zero integer — every row has a non-zero share of dW and db, and of the masked column sums — at 197 and at 1025
    rows alike; a bound of 1e-5 of a column's mass stops seeing one row near 1e5 rows."""
    narrow, colsum = M.GUARD_NARROW[1], next(c for c in M.COLSUM_LATTICE if (c.rows, c.H, c.mask, c.colsum_rows) == (1025, 64, True, 0))
    g, x = M.inputs(narrow)["g"].double(), M.inputs(narrow)["x"].double()
    masked = M.reference(colsum)["grad_in"]
    for row in range(narrow.rows):
        assert bool((g[row] != 0).any()) and bool((torch.outer(g[row], x[row]) != 0).any()), row  # its share of db and of dW
    for row in range(colsum.rows):
        assert bool((masked[row] != 0).any()), row  # its share of the column sums


@pytest.mark.parametrize("case", FLOAT, ids=M.ident)
def test_fp32_arithmetic_stays_inside_the_float_bounds(case):
    """Plain fp32 numpy (sequential and pairwise sums, in two orders) through the device test's own assertion."""
    import oracle

    for shuffled in (False, True):
        got = {name: torch.from_numpy(np.ascontiguousarray(value)) for name, value in _f32_outputs(case, shuffled).items()}
        M.check_float(case, got)
        if isinstance(case, M.InputLayer):
            assert oracle.gradient_error(got["dW"].numpy(), M.reference(case)["dW"].numpy()) <= M.INPUT_DW_BOUND
        if isinstance(case, M.Colsum):  # the mask itself is exact
            assert torch.equal(got["grad_in"].double(), M.reference(case)["grad_in"])


# ------------------------------------------------------------------------------------------------ the tables cover what they claim
def test_narrow_tables_cover_every_instantiation_and_edge():
    assert {(c.O, c.K, c.relu_input) for c in M.NARROW_LATTICE} == {(O, K, relu) for O in range(1, 17) for K in (32, 64, 128, 256, 512, 1024)
                                                                     for relu in (False, True)}
    assert all(c.rows == 197 and c.partials == 3 and c.rows - 2 * M.HEAD_ROWS == 5 and c.head_rows == 0 for c in M.NARROW_LATTICE)
    # O = 9: the first width with two rows in flight; O = 15: the first whose LDS passes 64 KB, at every K
    assert [M.narrow_in_flight(O) for O in (8, 9)] == [4, 2]
    assert all(M.narrow_lds_bytes(K, 14) <= 64 * 1024 < M.narrow_lds_bytes(K, 15) for K in M.KS)
    # K = 32: one pass of a block covers more rows than a default block holds; K = 1024: one row group
    assert M.narrow_groups(32) * M.narrow_in_flight(1) == 128 > M.HEAD_ROWS and M.narrow_groups(1024) == 1
    for K, O in ((32, 9), (128, 12), (1024, 15)):
        edges = [c for c in M.NARROW_ROW_EDGES if (c.K, c.O) == (K, O)]
        assert {c.rows for c in edges} == {1, 95, 96, 97, 192, 193} and {c.relu_input for c in edges} == {False, True}
        assert {c.rows: c.partials for c in edges} == {1: 1, 95: 1, 96: 1, 97: 2, 192: 2, 193: 3}
    assert {c.rows for c in M.NARROW_HEAD_ROWS} == {7, 8, 9, 127, 129} and all(c.K == 32 and c.head_rows == 8 for c in M.NARROW_HEAD_ROWS)
    assert M.narrow_groups(32) - 8 == 24  # row groups of a block that start past an 8-row block's end
    assert {M.narrow_in_flight(c.O) for c in M.NARROW_HEAD_ROWS} == {2, 4}
    for K, O in ((64, 3), (128, 16)):
        cases = [c for c in M.NARROW_FINALIZE if (c.K, c.O) == (K, O)]
        assert sorted(c.partials for c in cases) == list(M.P_EDGES) == [1, 15, 16, 17, 48, 49, 50, 64, 65, 100, 113, 128]
        assert all(c.rows % 8 == 5 and c.relu_input for c in cases)
    assert M.finalize_blocks(M.narrow_width(64, 3)) == 5 and M.narrow_width(64, 3) % 64 != 0  # a last block of 16 columns
    assert {(c.K, c.O) for c in M.NARROW_FLOAT} >= {(32, 9), (512, 15)}
    assert [(c.rows, c.K, c.O) for c in M.GUARD_NARROW] == [(197, 32, 9), (197, 128, 12), (97, 1024, 16)]


def test_finalize_edges_reach_the_unrolled_loop_and_its_tail():
    """P = 49 is the first count that enters the unrolled loop; 50, 65, 100, 113 leave a tail behind it; 64 and 128 none for
    group 0; 17 gives group 0 its second row."""
    assert [M.unrolled_passes(P) for P in M.P_EDGES] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2]
    for P in M.P_EDGES:
        counted = np.zeros(P, int)
        for group in range(M.FINALIZE_GROUPS):  # the loop of the vector finalize kernels, restated
            p = group
            while p + 48 < P:
                counted[[p, p + 16, p + 32, p + 48]] += 1
                p += 64
            while p < P:
                counted[p] += 1
                p += 16
        assert (counted == 1).all(), P


def test_row_dot_table_covers_every_form():
    assert {M.row_dot_lanes(K) for K in M.KS} == {8, 16, 32, 64} and {M.row_dot_rows_per_wave(K) for K in M.KS} == {32, 16, 8, 4}
    assert {(c.K, c.rows, c.bias) for c in M.ROW_DOT_LATTICE} == {(K, rows, bias) for K in M.KS for rows in (1, 3, 4, 5, 31, 32, 33, 1023, 1025)
                                                                  for bias in (True, False)}
    rows = {c.rows for c in M.ROW_DOT_LATTICE}
    assert {3, 4, 5} <= rows and {31, 32, 33} <= rows  # around one wave's rows of the 64-lane and the 8-lane form
    assert all(1024 % (4 * M.row_dot_rows_per_wave(K)) == 0 for K in M.KS)  # 1023 / 1025: one row around whole blocks
    assert [(c.rows, c.K) for c in M.GUARD_ROW_DOT] == [(33, 32), (1025, 256)]
    assert {M.row_dot_lanes(c.K) for c in M.ROW_DOT_FLOAT} >= {8, 64}


def test_input_layer_table_covers_every_edge():
    cases = M.INPUT_LATTICE
    assert {c.K for c in cases if c.H == 64 and c.rows == 37} == set(range(4, 61, 4))
    assert {(c.H, c.rows) for c in cases if c.K == 48 and c.rows != 37} == {(H, rows) for H in (64, 128, 320, 4096) for rows in (1, 15, 16, 17, 129)}
    assert sorted({c.partials for c in cases if "groups of the row sum" in c.edge}) == list(M.INPUT_ROW_BLOCKS) == [1, 2, 16, 17, 33, 64, 65]
    assert {c.mask for c in cases} == {True, False} and all(any(d == c._replace(mask=not c.mask, seed=d.seed) for d in cases) for c in cases)
    assert M.input_layer_row_blocks(24576, 256) == 64 and M.input_layer_row_blocks(8, 256) == 1  # (the figures the library is held to)
    assert [(c.rows, c.K, c.H) for c in M.GUARD_INPUT] == [(37, 60, 128)] * 2 and M.GUARD_INPUT[0].partials == 3


def test_colsum_table_puts_every_width_on_the_form_it_claims():
    cases = M.COLSUM_LATTICE
    assert all(M.colsum_chunked(H) for H in M.COLSUM_CHUNKED_H) and not any(M.colsum_chunked(H) for H in M.COLSUM_ROWWISE_H)
    assert M.COLSUM_CHUNKED_H == (4, 8, 16, 32, 64, 128, 256, 512, 1024) and M.COLSUM_ROWWISE_H == (1, 5, 12, 65, 100, 130, 1028)
    for case in cases:
        assert case.chunked == ("chunked" in case.edge or "finalize over" in case.edge), case
    assert {(c.H, c.rows, c.colsum_rows, c.mask) for c in cases if c.chunked and "finalize over" not in c.edge} == {
        (H, rows, cr, mask) for H in M.COLSUM_CHUNKED_H for rows in M.COLSUM_ROWS_SET for cr in (0, 4, 4096) for mask in (True, False)}
    assert {(c.H, c.rows, c.mask) for c in cases if not c.chunked} == {
        (H, rows, mask) for H in M.COLSUM_ROWWISE_H for rows in M.COLSUM_ROWS_SET for mask in (True, False)}
    assert M.COLSUM_ROWS_SET == (1, 63, 64, 65, 257, 1025)
    assert {M.finalize_blocks(H) for H in M.COLSUM_ROWWISE_H} >= {1, 2, 3}  # (65 and 100: two; 130: three)
    assert {c.partials for c in cases if not c.chunked} == {1, 2}  # 1025 rows: a second block of the row-wise kernel
    for H in (64, 256):
        edges = [c for c in cases if "finalize over" in c.edge and c.H == H and c.mask]
        assert sorted(c.partials for c in edges) == list(M.P_EDGES) and all(c.rows % 4 == 2 and c.colsum_rows == 4 for c in edges)
    assert {c.H for c in M.COLSUM_FLOAT} >= {512, 100}
    assert [(c.rows, c.H, c.mask) for c in M.GUARD_COLSUM] == [(257, 64, True), (257, 64, False), (257, 100, True), (257, 100, False), (65, 8, True)]


def test_cases_are_distinct_and_small():
    assert len({c.seed for c in M.ALL_CASES}) == len(M.ALL_CASES)
    for table in (M.NARROW_CASES, M.ROW_DOT_CASES, M.INPUT_CASES, M.COLSUM_CASES):
        assert len({c.name + c.values for c in table}) == len(table)
    assert max(c.rows for c in M.ALL_CASES) <= M.MAX_ROWS
    widest = max(c.rows * getattr(c, "H", getattr(c, "K", 0)) for c in M.ALL_CASES)
    assert widest * 4 <= 8 * 2**20  # no operand above 8 MB
