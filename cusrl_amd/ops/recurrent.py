"""Gate passes of one GRU / LSTM / RNN time step (``csrc/gru.hip``, ``recurrent.hip``)."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream


def gru_gates_forward(gi: torch.Tensor, gh: torch.Tensor, b_hh: torch.Tensor | None, h: torch.Tensor, out: torch.Tensor,
                      lengths: torch.Tensor | None, t: int) -> None:
    """One GRU time step's gate pass (``cusrl_gru_gates_fwd``): ``h`` [B, H] is advanced in place, ``out`` [B, H] gets the
    step's output; ``gi`` / ``gh`` are the [B, 3H] projections.  Called once per step of a sequence: the caller
    (nn/gru.py) guarantees contiguous fp32 device tensors, only shapes are checked here."""
    B, H = h.shape
    if gi.shape != (B, 3 * H) or gh.shape != (B, 3 * H) or out.shape != (B, H):
        raise ValueError("gru_gates_forward: shape mismatch")
    _checked.cusrl_gru_gates_fwd(gi.data_ptr(), gh.data_ptr(), _ptr(b_hh), h.data_ptr(), out.data_ptr(), _ptr(lengths), t, B, H, _stream())


def gru_gates_backward(gi: torch.Tensor, gh: torch.Tensor, b_hh: torch.Tensor | None, h_prev: torch.Tensor,
                       d_out: torch.Tensor | None, dh: torch.Tensor, lengths: torch.Tensor | None, t: int,
                       bias_partials: torch.Tensor | None = None) -> None:
    """Backward of :func:`gru_gates_forward`, in place: ``gi`` / ``gh`` become their gradients, ``dh`` (the gradient that
    arrived from step t + 1) becomes the direct-path gradient of ``h_prev`` (``cusrl_gru_gates_bwd``).  With
    ``bias_partials`` (``[gru_bias_partial_rows(B), 4H]`` = ``[ceil(B / rows), 4H]``, ``rows`` being the ``gru_bias_rows``
    option: 4 | 8 | 16 | 32, 16 unless set) every block of ``rows`` rows also leaves the column sums of the gate gradients it
    wrote — {d_r, d_z, d_n, d_q} — for the bias gradients (``cusrl_gru_gates_bwd_bias``)."""
    B, H = dh.shape
    if gi.shape != (B, 3 * H) or gh.shape != (B, 3 * H) or h_prev.shape != (B, H):
        raise ValueError("gru_gates_backward: shape mismatch")
    if bias_partials is not None:
        expected = (gru_bias_partial_rows(B), 4 * H)
        if bias_partials.shape != expected or not bias_partials.is_contiguous():
            raise ValueError(f"gru_gates_backward: 'bias_partials' must be a contiguous [ceil(B / gru_bias_rows), 4H] = "
                             f"{list(expected)} tensor, got {list(bias_partials.shape)}")
        _checked.cusrl_gru_gates_bwd_bias(gi.data_ptr(), gh.data_ptr(), _ptr(b_hh), h_prev.data_ptr(), _ptr(d_out), dh.data_ptr(),
                _ptr(lengths), t, B, H, bias_partials.data_ptr(), _stream())
        return
    _checked.cusrl_gru_gates_bwd(gi.data_ptr(), gh.data_ptr(), _ptr(b_hh), h_prev.data_ptr(), _ptr(d_out), dh.data_ptr(),
            _ptr(lengths), t, B, H, _stream())


def gru_bias_partials_supported(H: int, gi, gh, b_hh, h_prev, d_out, dh, bias_partials=None) -> bool:
    """Can :func:`gru_gates_backward` fold the bias gradients in?  Asked of the library (``cusrl_gru_bias_supported``: pointer
    alignment + column chunks that tile a 256-thread block); ``bias_partials=None``: a fresh allocation (256-byte aligned)."""
    return bool(_native.lib().cusrl_gru_bias_supported(H, _ptr(gi), _ptr(gh), _ptr(b_hh), _ptr(h_prev), _ptr(d_out), _ptr(dh),
                                                       bias_partials.data_ptr() if bias_partials is not None else 256))


def gru_bias_partial_rows(B: int) -> int:
    return int(_native.lib().cusrl_gru_bias_partial_rows(B))


def lstm_gates_forward(gi: torch.Tensor, gh: torch.Tensor, b_hh: torch.Tensor | None, h: torch.Tensor, c: torch.Tensor,
                       out: torch.Tensor, c_saved: torch.Tensor | None, lengths: torch.Tensor | None, t: int) -> None:
    """One LSTM time step's gate pass (``cusrl_lstm_gates_fwd``): ``h`` / ``c`` [B, H] advance in place, ``out`` gets the
    step's output; with ``c_saved`` (training) the new cell state is stored there and ``gi`` [B, 4H] is overwritten with
    the summed pre-activations the backward pass consumes."""
    B, H = h.shape
    if gi.shape != (B, 4 * H) or gh.shape != (B, 4 * H) or out.shape != (B, H) or c.shape != (B, H):
        raise ValueError("lstm_gates_forward: shape mismatch")
    _checked.cusrl_lstm_gates_fwd(gi.data_ptr(), gh.data_ptr(), _ptr(b_hh), h.data_ptr(), c.data_ptr(), out.data_ptr(),
            _ptr(c_saved), _ptr(lengths), t, B, H, _stream())


def lstm_gates_backward(pre: torch.Tensor, c_prev: torch.Tensor, c_next: torch.Tensor, d_out: torch.Tensor | None,
                        dh: torch.Tensor, dc: torch.Tensor, lengths: torch.Tensor | None, t: int) -> None:
    """Backward of :func:`lstm_gates_forward`, in place: ``pre`` becomes its gradient, ``dc`` the gradient of the previous
    cell state, ``dh`` the part of the state gradient that bypasses the step (``cusrl_lstm_gates_bwd``)."""
    B, H = dh.shape
    if pre.shape != (B, 4 * H) or c_prev.shape != (B, H) or c_next.shape != (B, H) or dc.shape != (B, H):
        raise ValueError("lstm_gates_backward: shape mismatch")
    _checked.cusrl_lstm_gates_bwd(pre.data_ptr(), c_prev.data_ptr(), c_next.data_ptr(), _ptr(d_out), dh.data_ptr(), dc.data_ptr(),
            _ptr(lengths), t, B, H, _stream())


def rnn_cell_forward(gi: torch.Tensor, gh: torch.Tensor, b_hh: torch.Tensor | None, h: torch.Tensor, out: torch.Tensor,
                     lengths: torch.Tensor | None, t: int, relu: bool) -> None:
    """One ``nn.RNN`` time step: ``h = act(gi + gh + b_hh)`` in place, ``out`` = the step's output (``cusrl_rnn_cell_fwd``)."""
    B, H = h.shape
    if gi.shape != (B, H) or gh.shape != (B, H) or out.shape != (B, H):
        raise ValueError("rnn_cell_forward: shape mismatch")
    _checked.cusrl_rnn_cell_fwd(gi.data_ptr(), gh.data_ptr(), _ptr(b_hh), h.data_ptr(), out.data_ptr(), _ptr(lengths),
            t, B, H, int(relu), _stream())


def rnn_cell_backward(d_pre: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor | None, dh: torch.Tensor,
                      lengths: torch.Tensor | None, t: int, relu: bool) -> None:
    """Backward of :func:`rnn_cell_forward`: ``d_pre`` receives the pre-activation gradient, ``dh`` keeps what bypasses the
    step (``cusrl_rnn_cell_bwd``)."""
    B, H = dh.shape
    if d_pre.shape != (B, H) or out.shape != (B, H):
        raise ValueError("rnn_cell_backward: shape mismatch")
    _checked.cusrl_rnn_cell_bwd(d_pre.data_ptr(), out.data_ptr(), _ptr(d_out), dh.data_ptr(), _ptr(lengths), t, B, H, int(relu), _stream())
