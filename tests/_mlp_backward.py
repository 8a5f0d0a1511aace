"""Shared by the tests of the MLP backward kernels — ``cusrl_narrow_linear_bwd`` / ``cusrl_narrow_linear_fwd``
(``csrc/narrow_linear.hip``), ``cusrl_input_layer_bwd`` (``input_layer.hip``) and ``cusrl_relu_bwd_colsum``
(``mlp_epilogue.hip``): tests/test_mlp_backward.py on the CPU, tests/test_mlp_backward_gpu.py on the device.  Imports no GPU.

Here: the float64 restatements of the four operations, the kernel constants the edge arithmetic needs (restated, so that a
changed default fails a test and does not quietly un-cover an edge), the expected partial counts, and the case tables.

The lattice.  ``lattice(shape, seed)`` draws integers in {-2, ..., 2} as fp32.  Every product of two entries is an integer of
magnitude <= 4 and every sum the kernels form — over at most 16 outputs, 1024 features or ``MAX_ROWS`` rows — an integer of
magnitude <= 4 * MAX_ROWS = 20000, far below 2^24: each intermediate is exactly representable in fp32, so ANY summation order,
any FMA contraction and the fp32 MFMA give the same bits, namely the int64 / float64 result cast to fp32.  The device assertion on
a lattice case is therefore ``torch.equal``: every element of every row counted exactly once, in the right slot.  (A dropped or
doubled row moves a sum by an integer; on random normals at the project's 1e-5-of-the-mass bound it can hide.)  ReLU outputs of
the lattice are exact zeros in about three entries of five, so ``> 0`` is decided at 0 itself.

Float cases draw standard normals and are held to the bounds the project already holds these kernels to: 1e-5 of each sum's
absolute mass (narrow backward, column sums), ``gradient_parity(..., 1e-5)`` for the input layer's dW and 1e-6 of the largest
column mass for its db, 4e-7 of sum |x| |w| for the row dot."""

from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ restated constants
BLOCK = 256            # threads of every kernel here but the input layer's
HEAD_ROWS = 96         # rows per block of the narrow backward (option "head_rows" = 0)
COLSUM_ROWS = 64       # rows per block of the chunked column-sum kernel (option "colsum_rows" = 0)
ROWWISE_ROWS = 1024    # rows per block of the row-wise column-sum kernel: 256 lanes x 4 rows
INPUT_CHUNK = 16       # rows of one chunk of the input-layer kernel (a block walks a multiple of it)
INPUT_COLUMNS = 64     # output columns per block of the input-layer kernel
INPUT_SUM_GROUPS = 16  # partial-row groups of input_layer_sum_rows_kernel
HEAD_PAD = 16          # floats of db padding behind the (O + 1) K floats of a narrow partial row
FINALIZE_GROUPS = 16   # partial-row groups of the vector finalize kernels; they unroll four rows while p + 48 < P
MAX_ROWS = 5000
KS = (32, 64, 128, 256, 512, 1024)
OS = tuple(range(1, 17))
P_EDGES = (1, 15, 16, 17, 48, 49, 50, 64, 65, 100, 113, 128)
UNSUPPORTED = -3       # CUSRL_E_UNSUPPORTED


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def narrow_partials(rows: int, head_rows: int = 0) -> int:
    """``cusrl_narrow_linear_num_partials``: one partial row per block of ``head_rows`` rows."""
    return ceil_div(rows, head_rows or HEAD_ROWS)


def narrow_width(K: int, O: int) -> int:
    """Floats of one partial row and of ``packed``: dW [O, K] | column sums of the masked dX [K] | db padded to 16."""
    return (O + 1) * K + HEAD_PAD


def narrow_groups(K: int) -> int:
    """Row groups of a narrow-backward block: a row takes K / 4 lanes."""
    return BLOCK // (K // 4)


def narrow_in_flight(O: int) -> int:
    return 2 if O > 8 else 4


def narrow_lds_bytes(K: int, O: int) -> int:
    """Dynamic LDS of the narrow backward: [groups][O + 1][K / 4] float4 and [groups][16] floats; above 64 KB the launch opts in."""
    return narrow_groups(K) * (O + 1) * (K // 4) * 16 + narrow_groups(K) * HEAD_PAD * 4


def row_dot_lanes(K: int) -> int:
    return min(64, K // 4)


def row_dot_rows_per_wave(K: int) -> int:
    """Rows one wave of the row-dot kernel owns: 64 / lanes row groups, four rows in flight each."""
    return 64 // row_dot_lanes(K) * 4


def colsum_chunked(H: int) -> bool:
    return H % 4 == 0 and H // 4 <= BLOCK and BLOCK % (H // 4) == 0


def colsum_partials(rows: int, H: int, colsum_rows: int = 0) -> int:
    """``cusrl_colsum_num_partials``."""
    return ceil_div(rows, colsum_rows or COLSUM_ROWS) if colsum_chunked(H) else ceil_div(rows, ROWWISE_ROWS)


def finalize_blocks(H: int) -> int:
    return ceil_div(H, 64)


def input_layer_rows_per_block(rows: int, H: int) -> int:
    row_blocks = max(ceil_div(256, H // INPUT_COLUMNS), ceil_div(rows, 512))
    row_blocks = min(row_blocks, ceil_div(rows, INPUT_CHUNK))
    return ceil_div(ceil_div(rows, row_blocks), INPUT_CHUNK) * INPUT_CHUNK


def input_layer_row_blocks(rows: int, H: int) -> int:
    """``cusrl_input_layer_row_blocks``."""
    return ceil_div(rows, input_layer_rows_per_block(rows, H))


def input_layer_width(K: int, H: int) -> int:
    return H * K + H


def unrolled_passes(P: int) -> int:
    """Passes group 0 of a vector finalize makes through its four-row unrolled loop (``p + 48 < P``, p += 64)."""
    return len(range(0, max(P - 48, 0), 64))


# ------------------------------------------------------------------------------------------------ inputs
def lattice(shape, seed: int) -> torch.Tensor:
    """fp32 integers drawn uniformly from {-2, ..., 2}."""
    return torch.from_numpy(np.random.default_rng(seed).integers(-2, 3, size=shape).astype(np.float32))


def normal(shape, seed: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------ float64 restatements
def _f64(t):
    return None if t is None else t.to(torch.float64)


def narrow_backward(g, x, w, relu_input: bool):
    """Backward of ``y = x w^T + b`` for at most 16 outputs: ``(dx, dW, db, colsum)``.  ``relu_input``: x is a ReLU's output;
    dx comes out masked by ``x > 0`` and ``colsum`` is its column sums (zeros otherwise: the slice the kernel leaves empty)."""
    g, x, w = _f64(g), _f64(x), _f64(w)
    dx = g @ w
    if relu_input:
        dx = dx * (x > 0)
    colsum = dx.sum(0) if relu_input else torch.zeros(x.shape[1], dtype=torch.float64)
    return dx, g.t() @ x, g.sum(0), colsum


def row_dot(x, w, b):
    out = _f64(x) @ _f64(w).t()
    return out if b is None else out + _f64(b)


def input_layer(g, y, x):
    """``(dW [H, K], db [H])`` of ``y = relu(x W^T + b)`` (``y`` None: no activation) for an input that needs no gradient."""
    masked = _f64(g) if y is None else _f64(g) * (y > 0)
    return masked.t() @ _f64(x), masked.sum(0)


def relu_colsum(g, y):
    """``(g', colsum)``: the ReLU's backward (``y`` None: none) and the column sums of what it passes."""
    masked = _f64(g) if y is None else _f64(g) * (y > 0)
    return masked, masked.sum(0)


# ------------------------------------------------------------------------------------------------ cases
class Narrow(NamedTuple):
    rows: int
    K: int
    O: int
    relu_input: bool
    head_rows: int  # 0: the default
    values: str     # lattice | normal
    edge: str
    seed: int

    @property
    def name(self) -> str:
        return f"r{self.rows}-K{self.K}-O{self.O}-{'relu' if self.relu_input else 'plain'}" + (f"-hr{self.head_rows}" if self.head_rows else "")

    @property
    def partials(self) -> int:
        return narrow_partials(self.rows, self.head_rows)


class RowDot(NamedTuple):
    rows: int
    K: int
    bias: bool
    values: str
    edge: str
    seed: int

    @property
    def name(self) -> str:
        return f"r{self.rows}-K{self.K}-{'bias' if self.bias else 'nobias'}"


class InputLayer(NamedTuple):
    rows: int
    K: int
    H: int
    mask: bool
    values: str
    edge: str
    seed: int

    @property
    def name(self) -> str:
        return f"r{self.rows}-K{self.K}-H{self.H}-{'mask' if self.mask else 'nomask'}"

    @property
    def partials(self) -> int:
        return input_layer_row_blocks(self.rows, self.H)


class Colsum(NamedTuple):
    rows: int
    H: int
    mask: bool
    colsum_rows: int  # 0: the default
    values: str
    edge: str
    seed: int

    @property
    def name(self) -> str:
        return f"r{self.rows}-H{self.H}-{'mask' if self.mask else 'nomask'}" + (f"-cr{self.colsum_rows}" if self.colsum_rows else "")

    @property
    def chunked(self) -> bool:
        return colsum_chunked(self.H)

    @property
    def partials(self) -> int:
        return colsum_partials(self.rows, self.H, self.colsum_rows)


_seed = [0]


def _next_seed() -> int:
    _seed[0] += 1
    return _seed[0]


def _narrow(rows, K, O, relu_input, edge, head_rows=0, values="lattice"):
    return Narrow(rows, K, O, relu_input, head_rows, values, edge, _next_seed())


def _colsum(rows, H, mask, edge, colsum_rows=0, values="lattice"):
    return Colsum(rows, H, mask, colsum_rows, values, edge, _next_seed())


def _input(rows, K, H, mask, edge, values="lattice"):
    return InputLayer(rows, K, H, mask, values, edge, _next_seed())


def _rows_for_row_blocks(blocks: int, H: int) -> int:
    """The smallest row count whose input-layer launch has ``blocks`` row blocks (its last block then holds a single row)."""
    return next(r for r in range(1, MAX_ROWS) if input_layer_row_blocks(r, H) == blocks)


# every instantiation: O in 1..16 (four rows in flight up to 8, two above; the 64 KB LDS opt-in from 15) at every K (32: 32 row
# groups, one pass of 128 rows > the 96-row block; 1024: one row group), three default blocks with a last one of 5 rows
NARROW_LATTICE = [_narrow(197, K, O, relu, f"instantiation O={O} K={K}, blocks of 96, 96, 5 rows") for O in OS for K in KS
                  for relu in (False, True)]
NARROW_ROW_EDGES = [_narrow(rows, K, O, relu, f"{rows} rows around the 96-row block at K={K} O={O}")
                    for K, O in ((32, 9), (128, 12), (1024, 15)) for rows in (1, 95, 96, 97, 192, 193) for relu in (False, True)]
# 8-row blocks under 32 row groups: 24 of the groups start past the block's end
NARROW_HEAD_ROWS = [_narrow(rows, 32, O, relu, f"head_rows=8 at K=32: {rows} rows", head_rows=8)
                    for O in (5, 9) for rows in (7, 8, 9, 127, 129) for relu in (False, True)]
# P partial rows of 8 rows, the last of 5: the finalize's unrolled loop, its tail, and a group's second row at P = 17
NARROW_FINALIZE = [_narrow(8 * P - 3, K, O, True, f"finalize over P={P} partial rows, {finalize_blocks(narrow_width(K, O))} blocks", head_rows=8)
                   for K, O in ((64, 3), (128, 16)) for P in P_EDGES]
NARROW_FLOAT = [_narrow(1000, 32, 9, True, "K=32, O=9: two rows in flight", values="normal"),
                _narrow(777, 512, 15, True, "K=512, O=15: the LDS opt-in", values="normal"),
                _narrow(197, 128, 12, False, "the policy head's shape, no ReLU in front", values="normal"),
                _narrow(509, 64, 3, True, "64 partial rows through the finalize", head_rows=8, values="normal")]
NARROW_CASES = NARROW_LATTICE + NARROW_ROW_EDGES + NARROW_HEAD_ROWS + NARROW_FINALIZE + NARROW_FLOAT

# the 8 / 16 / 32 / 64-lane forms; a wave owns 32 / 16 / 8 / 4 rows: 3, 4, 5 and 31, 32, 33 straddle those, 1023 / 1025 a block
ROW_DOT_LATTICE = [RowDot(rows, K, bias, "lattice", f"{row_dot_lanes(K)} lanes per row, {rows} rows", _next_seed())
                   for K in KS for rows in (1, 3, 4, 5, 31, 32, 33, 1023, 1025) for bias in (True, False)]
ROW_DOT_FLOAT = [RowDot(1025, 32, True, "normal", "8 lanes per row", _next_seed()),
                 RowDot(1023, 512, False, "normal", "64 lanes, two chunks per lane", _next_seed()),
                 RowDot(33, 1024, True, "normal", "64 lanes, four chunks per lane", _next_seed())]
ROW_DOT_CASES = ROW_DOT_LATTICE + ROW_DOT_FLOAT

INPUT_ROW_BLOCKS = (1, 2, 16, 17, 33, 64, 65)
INPUT_LATTICE = (
    [_input(37, K, 64, mask, f"K={K}: lanes 0..{K // 4 - 1} carry features, lane {K // 4} the ones") for K in range(4, 61, 4) for mask in (True, False)]
    + [_input(rows, 48, H, mask, f"H={H}: {H // 64} column groups, {rows} rows around the 16-row chunk") for H in (64, 128, 320, 4096)
       for rows in (1, 15, 16, 17, 129) for mask in (True, False)]
    + [_input(_rows_for_row_blocks(blocks, 64), 8, 64, mask, f"{blocks} partial rows over the 16 groups of the row sum")
       for blocks in INPUT_ROW_BLOCKS for mask in (True, False)])
INPUT_FLOAT = [_input(1000, 48, 320, True, "five column groups, ragged last block", values="normal"),
               _input(129, 60, 64, False, "K=60, no mask", values="normal")]
INPUT_CASES = INPUT_LATTICE + INPUT_FLOAT

COLSUM_CHUNKED_H = (4, 8, 16, 32, 64, 128, 256, 512, 1024)
COLSUM_ROWWISE_H = (1, 5, 12, 65, 100, 130, 1028)
COLSUM_ROWS_SET = (1, 63, 64, 65, 257, 1025)
COLSUM_LATTICE = (
    [_colsum(rows, H, mask, f"chunked H={H}: {BLOCK // (H // 4)} rows per pass, blocks of {cr or COLSUM_ROWS} rows, {rows} rows", colsum_rows=cr)
     for H in COLSUM_CHUNKED_H for rows in COLSUM_ROWS_SET for cr in (0, 4, 4096) for mask in (True, False)]
    + [_colsum(rows, H, mask, f"row-wise H={H}: {finalize_blocks(H)} finalize blocks, {rows} rows")
       for H in COLSUM_ROWWISE_H for rows in COLSUM_ROWS_SET for mask in (True, False)]
    + [_colsum(4 * P - 2, H, mask, f"finalize over P={P} partial rows, {finalize_blocks(H)} blocks", colsum_rows=4)
       for H in (64, 256) for P in P_EDGES for mask in (True, False)])
COLSUM_FLOAT = [_colsum(1025, 512, True, "chunked H=512: two rows per pass", values="normal"),
                _colsum(1025, 100, True, "row-wise H=100: two finalize blocks, two row blocks", values="normal"),
                _colsum(257, 16, False, "chunked H=16, no mask", values="normal"),
                _colsum(451, 256, True, "113 partial rows through the finalize", colsum_rows=4, values="normal")]
COLSUM_CASES = COLSUM_LATTICE + COLSUM_FLOAT

# one ragged multi-block shape per kernel and form for the guard-band tests (lattice values)
GUARD_NARROW = [_narrow(197, 32, 9, True, "guard"), _narrow(197, 128, 12, False, "guard"), _narrow(97, 1024, 16, True, "guard")]
GUARD_COLSUM = [_colsum(257, 64, True, "guard"), _colsum(257, 64, False, "guard"), _colsum(257, 100, True, "guard"),
                _colsum(257, 100, False, "guard"), _colsum(65, 8, True, "guard")]
GUARD_INPUT = [_input(37, 60, 128, True, "guard"), _input(37, 60, 128, False, "guard")]
GUARD_ROW_DOT = [RowDot(33, 32, True, "lattice", "guard", _next_seed()), RowDot(1025, 256, False, "lattice", "guard", _next_seed())]

ALL_CASES = NARROW_CASES + ROW_DOT_CASES + INPUT_CASES + COLSUM_CASES + GUARD_NARROW + GUARD_COLSUM + GUARD_INPUT + GUARD_ROW_DOT


def is_lattice(case) -> bool:
    return case.values == "lattice"


def ident(case) -> str:
    return case.name


# (small caches: the tests of one case share its tensors; the tables together would be hundreds of MB)
@functools.lru_cache(maxsize=4)
def inputs(case) -> dict:
    """The case's operands as fp32 CPU tensors (shared by the users of a case; nobody writes to them)."""
    draw = lattice if is_lattice(case) else normal
    seed = 16 * case.seed
    if isinstance(case, Narrow):
        x = draw((case.rows, case.K), seed + 1)
        return {"g": draw((case.rows, case.O), seed), "x": torch.relu(x) if case.relu_input else x, "w": draw((case.O, case.K), seed + 2)}
    if isinstance(case, RowDot):
        return {"x": draw((case.rows, case.K), seed), "w": draw((1, case.K), seed + 1), "b": draw((1,), seed + 2) if case.bias else None}
    if isinstance(case, InputLayer):
        return {"g": draw((case.rows, case.H), seed), "y": torch.relu(draw((case.rows, case.H), seed + 1)) if case.mask else None,
                "x": draw((case.rows, case.K), seed + 2)}
    return {"g": draw((case.rows, case.H), seed), "y": torch.relu(draw((case.rows, case.H), seed + 1)) if case.mask else None}


@functools.lru_cache(maxsize=4)
def reference(case) -> dict:
    """The float64 result of the case (shared like the inputs)."""
    data = inputs(case)
    if isinstance(case, Narrow):
        return dict(zip(("dx", "dW", "db", "colsum"), narrow_backward(data["g"], data["x"], data["w"], case.relu_input)))
    if isinstance(case, RowDot):
        return {"out": row_dot(data["x"], data["w"], data["b"])}
    if isinstance(case, InputLayer):
        return dict(zip(("dW", "db"), input_layer(data["g"], data["y"], data["x"])))
    return dict(zip(("grad_in", "colsum"), relu_colsum(data["g"], data["y"])))


@functools.lru_cache(maxsize=4)
def expected(case) -> dict:
    """The fp32 tensors a lattice case must produce, bit for bit."""
    assert is_lattice(case)
    return {name: value.to(torch.float32) for name, value in reference(case).items()}


# ------------------------------------------------------------------------------------------------ float bounds
MASS_BOUND = 1e-5     # of each sum's absolute mass: narrow backward, column sums
ROW_DOT_BOUND = 4e-7  # of sum |x| |w|
INPUT_DW_BOUND = 1e-5  # gradient_parity: of dW's largest entry
INPUT_DB_BOUND = 1e-6  # of the largest column mass


def masses(case) -> dict:
    """Per output the sum of the absolute values of the terms that enter each of its sums (float64)."""
    data = {name: None if value is None else value.double() for name, value in inputs(case).items()}
    if isinstance(case, Narrow):
        g, x, w = data["g"].abs(), data["x"].abs(), data["w"].abs()
        return {"dx": g @ w, "dW": g.t() @ x, "db": g.sum(0), "colsum": reference(case)["dx"].abs().sum(0)}
    if isinstance(case, RowDot):
        return {"out": data["x"].abs() @ data["w"].abs().t()}
    if isinstance(case, InputLayer):
        masked = relu_colsum(data["g"], data["y"])[0].abs()
        return {"db": masked.sum(0)}
    return {"colsum": reference(case)["grad_in"].abs().sum(0)}


def worst_fraction(got: torch.Tensor, want: torch.Tensor, mass: torch.Tensor) -> float:
    """max over the elements of |got - want| / mass (0 where the mass is 0 and the two agree)."""
    error = (got.double().cpu() - want).abs()
    assert bool((error[mass == 0] == 0).all())
    return float((error / mass.clamp_min(1e-300))[mass > 0].max()) if bool((mass > 0).any()) else 0.0


def check_float(case, got: dict) -> dict:
    """The float bounds of a ``normal`` case over ``got`` (fp32 tensors by output name), the input layer's dW excepted (the
    ``gradient_parity`` fixture takes it); returns the achieved fractions of each bound."""
    want, mass = reference(case), masses(case)
    used = {}
    if isinstance(case, InputLayer):
        scale = float(mass["db"].max())
        used["db"] = float((got["db"].double().cpu() - want["db"]).abs().max()) / (INPUT_DB_BOUND * scale)
    else:
        bound = ROW_DOT_BOUND if isinstance(case, RowDot) else MASS_BOUND
        for name in mass:
            used[name] = worst_fraction(got[name], want[name], mass[name]) / bound
    for name, fraction in used.items():
        print(f"{case.name}:{name}: {fraction:.3e} of its bound")
        assert fraction <= 1.0, f"{case.name}:{name}: {fraction:.3e} of its bound"
    return used
