"""``act(x + bias)`` over the columns of a ``[rows, H]`` matrix as one launch (``csrc/bias_act.hip``): the epilogue of a
bias-free GEMM.  Formulas and activation codes: include/cusrl_hip.h."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _modified_in_place, _stream

ACTIVATION_CODES = {
    "identity": _native._CONSTANTS["ACT_IDENTITY"],
    "relu": _native._CONSTANTS["ACT_RELU"],
    "elu": _native._CONSTANTS["ACT_ELU"],
    "tanh": _native._CONSTANTS["ACT_TANH"],
}


def bias_act_supported(x, bias) -> bool:
    """Does ``cusrl_bias_act`` take these operands?  ``x``: an fp32, contiguous, 2-D device tensor with at least one element;
    ``bias``: an fp32 contiguous vector of its width on the same device."""
    return (isinstance(x, torch.Tensor) and isinstance(bias, torch.Tensor) and x.is_cuda and x.dim() == 2 and x.numel() > 0
            and x.dtype == torch.float32 and x.is_contiguous() and bias.dtype == torch.float32 and bias.device == x.device
            and bias.shape == (x.shape[1],) and bias.is_contiguous())


def bias_act(x: torch.Tensor, bias: torch.Tensor, activation: str | int, alpha: float = 1.0,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """``act(x + bias)`` with ``activation`` one of ``"identity"``, ``"relu"``, ``"elu"`` (``alpha``), ``"tanh"`` (any letter
    case, or the header's integer code) — one launch, no gradient.  ``out`` may be ``x`` itself (in place) or another contiguous
    fp32 tensor of its shape; by default a new tensor.  Operands :func:`bias_act_supported` refuses raise: there is no torch
    form behind this entry."""
    if not bias_act_supported(x, bias):
        raise ValueError("bias_act: 'x' must be a non-empty contiguous fp32 [rows, H] device tensor and 'bias' a contiguous fp32 "
                         f"[H] vector beside it; got {_describe(x)} and {_describe(bias)}")
    if isinstance(activation, str):
        code = ACTIVATION_CODES.get(activation.lower())
        if code is None:
            raise ValueError(f"bias_act: unknown activation '{activation}'; expected one of {sorted(ACTIVATION_CODES)}")
    else:
        code = int(activation)  # (the library refuses a code it does not know)
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.shape == x.shape and out.dtype == torch.float32 and out.device == x.device
              and out.is_contiguous()):
        raise ValueError(f"bias_act: 'out' must be a contiguous fp32 tensor shaped like 'x'; got {_describe(out)}")
    _checked.cusrl_bias_act(x.data_ptr(), bias.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], code, float(alpha), _stream())
    if out is x or out.data_ptr() == x.data_ptr():
        _modified_in_place(out)
    return out


def _describe(value) -> str:
    if not isinstance(value, torch.Tensor):
        return type(value).__name__
    return f"{value.dtype} {tuple(value.shape)} on {value.device}{'' if value.is_contiguous() else ' (strided)'}"
