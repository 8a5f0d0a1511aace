"""The inputs of the exact device tests of ``cusrl_mlp2_forward`` and ``cusrl_narrow_linear_fwd`` (tests/test_mlp_forward_gpu.py),
checked on the CPU: for every shape those tests draw an integer stack at, the accumulated magnitude stays below 2^24, torch's
fp32 chain on the host equals float64 to the bit, and between 20 % and 80 % of either hidden layer is live behind its ReLU.
These are conditions on the inputs, taken from the reference alone — they are what entitles the device tests to
``torch.equal``.  If one fails, the draw (tests/_mlp_forward.py) is to be changed, not the condition."""

from __future__ import annotations

import pytest
import torch

import _mlp_forward as M


def _ident(shape) -> str:
    K, H1, H2, rows, seed, bias3 = shape
    return f"{K}-{H1}-{H2}-r{rows}-s{seed}" + ("" if bias3 else "-nobias")


def test_the_shape_table_reaches_every_instantiation():
    small = {M.instantiation(K, H1, H2) for K, H1, H2, rows, _, _ in M.integer_shapes() if rows == M.ROWS_SMALL}
    assert small == {f"<{t1},{t2},{kb}>" for t1 in (2, 4) for t2 in (1, 2) for kb in (1, 2, 3, 4)}
    assert {M.instantiation(K, H1, H2) for H1, H2 in M.HIDDEN for K in M.K_FLOAT} == small
    assert [M.instantiation(*s) for s in M.ROW_EDGE_STACKS] == ["<4,2,3>", "<2,1,4>"]
    assert [M.instantiation(*s[:3]) for s in M.INDEPENDENCE_STACKS] == ["<4,2,3>", "<2,2,2>"]
    assert [M.instantiation(*s) for s in M.SAMPLING_STACKS] == ["<4,2,3>", "<2,1,1>", "<4,1,4>"]


@pytest.mark.parametrize("shape", M.integer_shapes(), ids=_ident)
def test_integer_stack_is_exact_in_fp32_and_cuts_both_ways(shape):
    K, H1, H2, rows, seed, bias3 = shape
    x, layers = M.integer_stack(K, H1, H2, M.MAX_OUT, rows, seed, bias3)
    assert x.dtype == torch.float32 and x.shape == (rows, K) and bool((x == x.round()).all()) and float(x.abs().max()) <= 2
    for weight in layers[0::2]:
        assert weight.dtype == torch.float32 and set(weight.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for bias in layers[1::2]:
        assert bias is None or (bool((bias == bias.round()).all()) and float(bias.abs().max()) <= 2)
    assert (layers[5] is None) == (not bias3)
    ref = M.integer_reference(*shape)
    assert float(ref["mag"].max()) < 2 ** 24
    assert ref["host_exact"], "torch's fp32 chain on the host differs from float64"
    assert all(0.2 <= share <= 0.8 for share in ref["live"]), ref["live"]
    M.check_integer_conditions(ref)  # (the same three, as the device tests ask them)
    # a head of A outputs is the first A columns of the A = 16 evaluation
    for A in (1, 5, 12):
        xa, la = M.integer_stack(K, H1, H2, A, rows, seed, bias3)
        out, mag = M._reference(xa, la)
        assert torch.equal(out, ref["out"][:, :A]) and torch.equal(mag, ref["mag"][:, :A])
        assert torch.equal(M.library_chain(xa, la).double(), out)


@pytest.mark.parametrize("K", M.ROW_DOT_KS)
def test_integer_row_dot_is_exact_in_fp32(K):
    for rows in M.ROW_DOT_ROWS:
        for bias in (True, False):
            x, w, b = M.integer_row_dot(K, rows, 4, bias)
            assert float(x.abs().max()) <= 2 and set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and (b is None) == (not bias)
            want = M.row_dot_reference(x, w, b)
            mass = x.double().abs() @ w.double().abs().T + (0 if b is None else b.double().abs())
            assert float(mass.max()) <= 2 * K + 2 <= 2050
            host = x @ w.T if b is None else x @ w.T + b
            assert torch.equal(host.double(), want)
