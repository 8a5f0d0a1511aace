"""Shared by the tests of the one-launch MLP inference pass ``cusrl_mlp2_forward`` (``csrc/mlp_forward.hip``) and of the
one-output row dot ``cusrl_narrow_linear_fwd`` (``csrc/narrow_linear.hip``): tests/test_mlp_forward.py and
tests/test_mlp_forward_gpu.py on the device, tests/test_mlp_forward_exact.py on the CPU.  Imports no GPU.

The integer stack.  ``integer_stack`` draws x and every bias from {-2, ..., 2} and every weight from {-1, 0, 1}, as fp32.  The
magnitude the three layers accumulate is then at most 128 (256 (64 * 2 + 2) + 2) + 2 = 4 260 098 < 2^24, so every product and
every partial sum of every layer — in ANY summation order, with or without FMA contraction, inside the MFMA or outside it — is
an integer fp32 represents exactly: a correct kernel returns the float64 result to the bit and the device assertion is
``torch.equal``.  A dropped, doubled or misplaced term moves a sum by an integer; on random normals it can hide inside a
relative bound.  The hidden pre-activations are symmetric around zero, so about half of each hidden layer is cut by its ReLU
and both of its sides are exercised (tests/test_mlp_forward_exact.py asserts the share for every shape the GPU tests use).

The head of an integer stack with A outputs is the first A rows of one [16, H2] draw (and the first A of 16 biases), everything
below the head does not depend on A: one float64 evaluation at A = 16 (``integer_reference``) serves every head width, by
slicing columns."""

from __future__ import annotations

import functools

import numpy as np
import torch

MAX_OUT = 16
EXACT = float(1 << 24)   # integers below it are fp32 values, and so are their sums
NOMINAL_CUS = 256        # compute units of an MI355X: the row counts the CPU test checks (the GPU tests ask the device)
UNSUPPORTED = -3         # CUSRL_E_UNSUPPORTED

HIDDEN = ((256, 128), (256, 64), (128, 128), (128, 64))   # <T1, T2> = <4,2> <4,1> <2,2> <2,1>
K_EDGES = (4, 16, 20, 32, 36, 48, 52, 64)                 # per k-block count: one live quad in the last block, a full last block
K_FLOAT = (12, 28, 48, 64)                                # one per k-block count
ROWS_SMALL = 37
ROW_EDGES = (1, 15, 16, 17, 31, 33)
ROW_DOT_KS = (32, 64, 128, 256, 512, 1024)
ROW_DOT_ROWS = (1, 7, 255, 256, 257, 4099)


def instantiation(K: int, H1: int, H2: int) -> str:
    """The ``mlp2_forward_kernel<T1, T2, KB>`` a shape is dispatched to."""
    return f"<{H1 // 64},{H2 // 64},{-(-K // 16)}>"


def grid_rows(cus: int) -> tuple[int, int, int]:
    """Row counts around the persistent loop of a grid of ``cus`` workgroups over 16-row tiles: exactly full; one workgroup walks
    two tiles (its look-ahead load clamped to the last tile); every workgroup walks more than one tile."""
    return 16 * cus, 16 * cus + 1, 32 * cus + 5


# ------------------------------------------------------------------------------------------------ float data
def stack(K, H1, H2, A, seed, bias3=True, device="cpu"):
    """(w1, b1, w2, b2, w3, b3) of normals scaled so that every layer's output is of order one."""
    g = torch.Generator().manual_seed(seed)
    make = lambda *shape, scale: (torch.randn(*shape, generator=g) * scale).to(device)  # noqa: E731
    return (make(H1, K, scale=K ** -0.5), make(H1, scale=0.3), make(H2, H1, scale=H1 ** -0.5), make(H2, scale=0.3),
            make(A, H2, scale=H2 ** -0.5), make(A, scale=0.3) if bias3 else None)


def _reference(x, layers):
    """float64, plus the magnitude the fp32 sums accumulate: |w3| (|w2| relu(...) + |b2|) + |b3| — the yardstick of the bound."""
    w1, b1, w2, b2, w3, b3 = [None if t is None else t.double().cpu() for t in layers]
    x = x.double().cpu()
    h1 = torch.relu(x @ w1.T + b1)
    h2 = torch.relu(h1 @ w2.T + b2)
    out = h2 @ w3.T + (0 if b3 is None else b3)
    m1 = x.abs() @ w1.abs().T + b1.abs()
    m2 = m1 @ w2.abs().T + b2.abs()
    mag = m2 @ w3.abs().T + (0 if b3 is None else b3.abs())
    return out, mag


def library_chain(x, layers):
    """The fp32 chain the unfused path runs, on the device of its operands."""
    w1, b1, w2, b2, w3, b3 = layers
    out = torch.relu(torch.relu(x @ w1.T + b1) @ w2.T + b2) @ w3.T
    return out if b3 is None else out + b3


# ------------------------------------------------------------------------------------------------ integer data
def _integers(rng, low, high, *shape) -> torch.Tensor:
    return torch.from_numpy(rng.integers(low, high + 1, size=shape).astype(np.float32))


@functools.lru_cache(maxsize=8)
def _integer_draw(K, H1, H2, rows, seed):
    rng = np.random.default_rng([K, H1, H2, rows, seed])
    x = _integers(rng, -2, 2, rows, K)
    w1, b1 = _integers(rng, -1, 1, H1, K), _integers(rng, -2, 2, H1)
    w2, b2 = _integers(rng, -1, 1, H2, H1), _integers(rng, -2, 2, H2)
    w3, b3 = _integers(rng, -1, 1, MAX_OUT, H2), _integers(rng, -2, 2, MAX_OUT)
    return x, (w1, b1, w2, b2, w3, b3)


def integer_stack(K, H1, H2, A, rows, seed, bias3=True):
    """``(x, (w1, b1, w2, b2, w3, b3))`` as fp32 CPU tensors of small integers (nobody writes to them): x and the biases in
    {-2..2}, the weights in {-1, 0, 1}; ``b3`` is None without ``bias3``.  Only the head depends on A (its first A rows)."""
    x, (w1, b1, w2, b2, w3, b3) = _integer_draw(K, H1, H2, rows, seed)
    return x, (w1, b1, w2, b2, w3[:A].contiguous(), b3[:A].contiguous() if bias3 else None)


@functools.lru_cache(maxsize=8)
def integer_reference(K, H1, H2, rows, seed, bias3=True) -> dict:
    """The float64 evaluation of the integer stack at A = 16 — ``out`` and ``mag`` ([rows, 16]: a head of A outputs is the
    first A columns), the share of each hidden layer that is live behind its ReLU, and whether torch's fp32 chain on the
    host equals float64 to the bit."""
    x, layers = integer_stack(K, H1, H2, MAX_OUT, rows, seed, bias3)
    out, mag = _reference(x, layers)
    w1, b1, w2, b2 = [t.double() for t in layers[:4]]
    h1 = torch.relu(x.double() @ w1.T + b1)
    h2 = torch.relu(h1 @ w2.T + b2)
    return {"label": f"{K}->{H1}->{H2} at {rows} rows, seed {seed}", "out": out, "mag": mag,
            "live": (float((h1 > 0).double().mean()), float((h2 > 0).double().mean())),
            "host_exact": torch.equal(library_chain(x, layers).double(), out)}


def check_integer_conditions(ref: dict) -> None:
    """The three conditions that make ``torch.equal`` the device assertion on an integer stack.  They are conditions on the
    INPUTS and come from the reference alone: if one fails the draw is to be changed, not the condition."""
    label, largest = ref["label"], float(ref["mag"].max())
    assert largest < EXACT, f"{label}: accumulated magnitude {largest:.0f} reaches 2^24"
    assert ref["host_exact"], f"{label}: the fp32 chain on the host differs from float64"
    assert all(0.2 <= share <= 0.8 for share in ref["live"]), f"{label}: live shares {ref['live']} outside 20-80 %"


def integer_expected(K, H1, H2, A, rows, seed, bias3=True) -> torch.Tensor:
    """float64 ``[rows, A]``: what every correct fp32 evaluation of ``integer_stack(K, H1, H2, A, rows, seed, bias3)`` returns
    (the conditions checked first)."""
    ref = integer_reference(K, H1, H2, rows, seed, bias3)
    check_integer_conditions(ref)
    return ref["out"][:, :A]


def integer_row_dot(K, rows, seed, bias=True):
    """``(x [rows, K] in {-2..2}, w [1, K] in {-1, 0, 1}, b [1] in {-2..2} or None)``: |sum| <= 2 K + 2 <= 2050, exact in fp32."""
    rng = np.random.default_rng([K, rows, seed])
    x, w, b = _integers(rng, -2, 2, rows, K), _integers(rng, -1, 1, 1, K), _integers(rng, -2, 2, 1)
    return x, w, (b if bias else None)


def row_dot_reference(x, w, b) -> torch.Tensor:
    out = x.double() @ w.double().T
    return out if b is None else out + b.double()


# ------------------------------------------------------------------------------------------------ the shapes the GPU tests use
ROW_EDGE_STACKS = ((48, 256, 128), (64, 128, 64))                  # <4,2,3> and <2,1,4>
INDEPENDENCE_STACKS = ((48, 256, 128, 12), (32, 128, 128, 5))      # <4,2,3> and <2,2,2>, with A
SAMPLING_STACKS = ((48, 256, 128), (16, 128, 64), (64, 256, 64))   # <4,2,3>, <2,1,1> and <4,1,4>
GUARD_STACK = (48, 256, 128)                                       # <4,2,3>
GUARD_OUTS = (1, 3, 5, 7, 12, 13, 16)


def sampling_rows(cus: int) -> tuple[int, int, int]:
    return 1, 17, 16 * cus + 1


def integer_shapes(cus: int = NOMINAL_CUS) -> list[tuple]:
    """Every ``(K, H1, H2, rows, seed, bias3)`` the GPU tests draw an integer stack at (each at every head width 1..16)."""
    shapes = []
    for H1, H2 in HIDDEN:                      # all 16 instantiations, both ends of every k-block count
        for K in K_EDGES:
            shapes += [(K, H1, H2, ROWS_SMALL, 1, True), (K, H1, H2, ROWS_SMALL, 1, False)]
    for K, H1, H2 in ROW_EDGE_STACKS:          # the row residues and the grid edges
        shapes += [(K, H1, H2, rows, 2, True) for rows in ROW_EDGES + grid_rows(cus)]
    for K, H1, H2 in SAMPLING_STACKS:          # the sampling epilogue
        shapes += [(K, H1, H2, rows, 3, True) for rows in sampling_rows(cus)]
    return shapes
