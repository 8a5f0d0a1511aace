"""The float64 single-step references of the recurrent gate passes (``oracle.gru_gates_step`` ... ``rnn_cell_step_backward``),
pinned without a GPU: the backward ones against float64 autograd of torch's cell equations, the forward ones — chained over
a sequence — against the sequence oracles that the reference's recordings pin.  Then every case of the GPU tests
(tests/test_recurrent_gates_gpu.py) is run through a float32 numpy restatement and the GPU tests' own assertions: correct fp32
arithmetic stays inside the bounds the kernels are held to."""

import numpy as np
import pytest
import torch

import _recurrent_gates as G
import oracle

T = 2


def _lengths(kind, B):
    return None if kind == "none" else np.array([(T + 3, T + 1, T, T - 1, 0)[b % 5] for b in range(B)], np.int64)


def _live(lengths, B):
    live = np.ones(B) if lengths is None else (T < lengths).astype(np.float64)
    return torch.from_numpy(live)[:, None]


def _leaves(rng, *shapes):
    return [torch.from_numpy(rng.standard_normal(shape)).requires_grad_() for shape in shapes]


def _close(label, got, want):
    error = oracle.gradient_error(got, want.detach().numpy() if isinstance(want, torch.Tensor) else want)
    assert error <= 1e-12, f"{label}: {error:.3e} of the largest entry"


OPTIONS = [(b, d, l) for b in (True, False) for d in (True, False) for l in ("none", "mixed")]


@pytest.mark.parametrize("with_bias,with_d_out,lengths_kind", OPTIONS)
def test_gru_backward_reference_is_the_autograd_gradient(with_bias, with_d_out, lengths_kind):
    B, H = 10, 6
    rng = np.random.default_rng(1)
    gi, gh, b, h = _leaves(rng, (B, 3 * H), (B, 3 * H), (3 * H,), (B, H))
    w_out, w_state = rng.standard_normal((B, H)), rng.standard_normal((B, H))
    lengths = _lengths(lengths_kind, B)
    live = _live(lengths, B)
    # torch.nn.GRU's cell: r, z = sigmoid(W_i x + b_i + W_h h + b_h), n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h
    hidden = gh + b if with_bias else gh
    r = torch.sigmoid(gi[:, :H] + hidden[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + hidden[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * hidden[:, 2 * H:])
    nxt = (1 - z) * n + z * h
    state, out = live * nxt + (1 - live) * h, live * nxt
    loss = (state * torch.from_numpy(w_state)).sum() + ((out * torch.from_numpy(w_out)).sum() if with_d_out else 0.0)
    want = torch.autograd.grad(loss, [gi, gh, h] + ([b] if with_bias else []))
    numpy = lambda v: v.detach().numpy()  # noqa: E731
    d_gi, d_gh, dh, sums = oracle.gru_gates_step_backward(numpy(gi), numpy(gh), numpy(b) if with_bias else None, numpy(h),
                                                          w_out if with_d_out else None, w_state, lengths, T)
    _close("d_gi", d_gi, want[0]), _close("d_gh", d_gh, want[1]), _close("dh", dh, want[2])
    _close("sums{r,z,n}", sums[:3 * H], want[0].sum(0))
    _close("sums{r,z,q}", np.concatenate([sums[:2 * H], sums[3 * H:]]), want[3] if with_bias else want[1].sum(0))
    got_h, got_out = oracle.gru_gates_step(numpy(gi), numpy(gh), numpy(b) if with_bias else None, numpy(h), lengths, T)
    _close("h", got_h, state), _close("out", got_out, out)
    if lengths is not None:
        dead = T >= lengths
        assert not d_gi[dead].any() and not d_gh[dead].any() and np.array_equal(dh[dead], w_state[dead])


@pytest.mark.parametrize("with_bias,with_d_out,lengths_kind", OPTIONS)
def test_lstm_backward_reference_is_the_autograd_gradient(with_bias, with_d_out, lengths_kind):
    B, H = 10, 6
    rng = np.random.default_rng(2)
    gi, gh, b, h, c = _leaves(rng, (B, 4 * H), (B, 4 * H), (4 * H,), (B, H), (B, H))
    w_out, w_h, w_c = (rng.standard_normal((B, H)) for _ in range(3))
    lengths = _lengths(lengths_kind, B)
    live = _live(lengths, B)
    # torch.nn.LSTM's cell: i, f, o = sigmoid, g = tanh of W_i x + b_i + W_h h + b_h; c' = f c + i g; h' = o tanh(c')
    pre = gi + gh + b if with_bias else gi + gh
    i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
    c_new = f * c + i * g
    h_new = o * torch.tanh(c_new)
    h_state, c_state, out = live * h_new + (1 - live) * h, live * c_new + (1 - live) * c, live * h_new
    loss = (h_state * torch.from_numpy(w_h)).sum() + (c_state * torch.from_numpy(w_c)).sum()
    if with_d_out:
        loss = loss + (out * torch.from_numpy(w_out)).sum()
    want = torch.autograd.grad(loss, [gi, gh, h, c])
    numpy = lambda v: v.detach().numpy()  # noqa: E731
    got_h, got_c, got_out, saved_pre, saved_c = oracle.lstm_gates_step(numpy(gi), numpy(gh), numpy(b) if with_bias else None,
                                                                       numpy(h), numpy(c), lengths, T)
    _close("h", got_h, h_state), _close("c", got_c, c_state), _close("out", got_out, out), _close("pre", saved_pre, pre)
    assert np.array_equal(saved_c, got_c)
    d_pre, dh, dc = oracle.lstm_gates_step_backward(saved_pre, numpy(c), saved_c, w_out if with_d_out else None, w_h, w_c, lengths, T)
    _close("d_pre", d_pre, want[0]), _close("d_pre (gh)", d_pre, want[1]), _close("dh", dh, want[2]), _close("dc", dc, want[3])
    if lengths is not None:
        dead = T >= lengths
        assert not d_pre[dead].any() and np.array_equal(dh[dead], w_h[dead]) and np.array_equal(dc[dead], w_c[dead])
        assert not dh[~dead].any()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias,with_d_out,lengths_kind", OPTIONS)
def test_rnn_backward_reference_is_the_autograd_gradient(with_bias, with_d_out, lengths_kind, relu):
    B, H = 10, 6
    rng = np.random.default_rng(3)
    gi, gh, b, h = _leaves(rng, (B, H), (B, H), (H,), (B, H))
    w_out, w_state = rng.standard_normal((B, H)), rng.standard_normal((B, H))
    lengths = _lengths(lengths_kind, B)
    live = _live(lengths, B)
    pre = gi + gh + b if with_bias else gi + gh  # torch.nn.RNN's cell: h' = tanh | relu(W_i x + b_i + W_h h + b_h)
    nxt = torch.relu(pre) if relu else torch.tanh(pre)
    state, out = live * nxt + (1 - live) * h, live * nxt
    loss = (state * torch.from_numpy(w_state)).sum() + ((out * torch.from_numpy(w_out)).sum() if with_d_out else 0.0)
    want = torch.autograd.grad(loss, [gi, gh, h])
    numpy = lambda v: v.detach().numpy()  # noqa: E731
    got_h, got_out = oracle.rnn_cell_step(numpy(gi), numpy(gh), numpy(b) if with_bias else None, numpy(h), lengths, T, relu)
    _close("h", got_h, state), _close("out", got_out, out)
    d_pre, dh = oracle.rnn_cell_step_backward(numpy(nxt), w_out if with_d_out else None, w_state,
                                              lengths, T, relu)
    _close("d_pre", d_pre, want[0]), _close("d_pre (gh)", d_pre, want[1]), _close("dh", dh, want[2])
    if lengths is not None:
        dead = T >= lengths
        assert not d_pre[dead].any() and np.array_equal(dh[dead], w_state[dead]) and not dh[~dead].any()


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("with_lengths", [False, True])
def test_chained_forward_references_are_the_sequence_oracles(with_bias, with_lengths):
    """One layer with an identity input projection (gi = x) and a given W_hh: the single-step functions, chained over L = 4
    steps, reproduce ``gru_sequence`` / ``lstm_sequence`` / ``rnn_sequence`` — which tests/golden/recurrent*.npz pin to the
    reference — bit for bit."""
    L, B, H = 4, 5, 6
    rng = np.random.default_rng(4)
    lengths = np.array([4, 1, 3, 2, 4], np.int64) if with_lengths else None
    h0, c0 = (rng.standard_normal((1, B, H)).astype(np.float32) for _ in range(2))
    for cell, gates in G.GATES.items():
        x = rng.standard_normal((L, B, gates * H)).astype(np.float32)
        w_hh = (rng.standard_normal((gates * H, H)) * 0.4).astype(np.float32)
        b_hh = rng.standard_normal(gates * H).astype(np.float32) if with_bias else None
        # (the identity projection maps an input of width gates * H to the gate pre-activations: a non-square "W_ih" of the
        # layer's hidden size is not needed — the sequence functions read H off W_hh)
        weights = [(np.eye(gates * H, dtype=np.float32), w_hh, None, b_hh)]
        for relu in ((False, True) if cell == "rnn" else (False,)):
            h, c, outs = h0[0].astype(np.float64), c0[0].astype(np.float64), []
            for t in range(L):
                gh = h @ w_hh.astype(np.float64).T
                if cell == "gru":
                    h, out = oracle.gru_gates_step(x[t], gh, b_hh, h, lengths, t)
                elif cell == "lstm":
                    h, c, out, _, _ = oracle.lstm_gates_step(x[t], gh, b_hh, h, c, lengths, t)
                else:
                    h, out = oracle.rnn_cell_step(x[t], gh, b_hh, h, lengths, t, relu)
                outs.append(out)
            if cell == "gru":
                want_out, want_h = oracle.gru_sequence(x, h0, weights, lengths)
            elif cell == "lstm":
                want_out, (want_h, want_c) = oracle.lstm_sequence(x, (h0, c0), weights, lengths)
                assert np.array_equal(c.astype(np.float32), want_c[0])
            else:
                want_out, want_h = oracle.rnn_sequence(x, h0, weights, lengths, relu=relu)
            assert np.array_equal(np.stack(outs).astype(np.float32), want_out), cell
            assert np.array_equal(h.astype(np.float32), want_h[0]), cell


def _restated(gradient_parity):
    """The GPU tests' ``gradient_parity`` with the records of this file kept in families of their own."""
    return lambda case: G.exercise(case, G.F32, gradient_parity, G.FAMILY[case.cell] + "_fp32_restatement")


@pytest.mark.parametrize("case", [case for cell in G.GATES for case in G.PLAIN[cell]], ids=lambda case: case.name)
def test_fp32_restatement_passes_the_gpu_assertions(case, gradient_parity):
    _restated(gradient_parity)(case)


@pytest.mark.parametrize("rows", G.BIAS_ROWS)
def test_fp32_restatement_of_the_bias_folding_pass_passes_the_gpu_assertions(rows, gradient_parity):
    cases = G.bias_cases(rows)
    assert cases
    for case in cases:
        _restated(gradient_parity)(case)


def test_case_matrix_covers_the_dispatch_edges():
    """The shapes the dispatch turns on are in the case list (a guard against an edit that drops one)."""
    for cell in G.GATES:
        shapes = {(case.B, case.H) for case in G.PLAIN[cell]}
        assert {(6, 8), (6, 5), (6, 7), (3, 1), (1, 8), (1, 5)} <= shapes
        assert {(B, 5) for B in (50, 51, 52)} | {(B, 16) for B in (63, 64, 65)} | {(B, 4) for B in (256, 257, 258)} <= shapes
        options = {(case.b_hh, case.d_out, case.lengths) for case in G.PLAIN[cell]}
        assert {(b, d, l) for b in (True, False) for d in (True, False) for l in ("none", "mixed")} <= options
        assert {"ended", "live"} <= {case.lengths for case in G.PLAIN[cell]} and {0, 23} <= {case.t for case in G.PLAIN[cell]}
    eligible = {(rows, case.H, case.form) for rows in G.BIAS_ROWS for case in G.bias_cases(rows)}
    assert (32, 32, "vec") in eligible and (4, 256, "vec") in eligible and (0, 1024, "vec") in eligible and (8, 32, "scalar") in eligible
    assert (16, 32, "vec") not in eligible and not any(H in (2048, 12, 5, 4) for _, H, _ in eligible)
    for data in (G.inputs(case) for case in G.PLAIN["gru"] if case.lengths == "mixed" and case.B >= 4):
        t, lengths = data["t"], data["lengths"]
        assert (t < lengths - 1).any() and (t == lengths - 1).any() and (t == lengths).any() and ((t > lengths).any() or t == 0)
