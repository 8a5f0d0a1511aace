"""The element-wise work of the gate layers and the GLU activations as one launch per direction (``csrc/gate.hip``): what sits
between the GEMMs of ``cusrl_amd.nn.gate`` and ``cusrl_amd.nn.activation``.  Formulas: include/cusrl_hip.h."""

from __future__ import annotations

import torch
from torch.nn.functional import gelu, silu

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _ptr, _stream

# kind -> (the header's constant, takes y, takes q)
GATE_KINDS = {
    "input": (_native._CONSTANTS["GATE_INPUT"], True, False),
    "output": (_native._CONSTANTS["GATE_OUTPUT"], True, False),
    "highway": (_native._CONSTANTS["GATE_HIGHWAY"], True, False),
    "sigmoid_tanh": (_native._CONSTANTS["GATE_SIGMOID_TANH"], False, True),
    "gru_reset": (_native._CONSTANTS["GATE_GRU_RESET"], False, False),
    "gru_out": (_native._CONSTANTS["GATE_GRU_OUT"], False, True),
}
GLU_KINDS = {"geglu": _native._CONSTANTS["GLU_GEGLU"], "swiglu": _native._CONSTANTS["GLU_SWIGLU"]}


def _operands(kind: str, x, y, p, q, p2, q2):
    """``(x, y, p, q, p2, q2)`` with what ``kind`` does not take dropped; a missing operand it does take is an error."""
    if kind not in GATE_KINDS:
        raise ValueError(f"Unknown gate kind '{kind}'; available kinds: {', '.join(map(repr, GATE_KINDS))}")
    _, takes_y, takes_q = GATE_KINDS[kind]
    if x is None or p is None or (takes_y and y is None) or (takes_q and q is None):
        raise ValueError(f"gate kind '{kind}' needs x, p{', y' if takes_y else ''}{', q' if takes_q else ''}")
    return x, (y if takes_y else None), p, (q if takes_q else None), p2, (q2 if takes_q else None)


def _launchable(tensors) -> bool:
    """fp32 device tensors right now: no autocast, and no differentiated forward inside ``double_differentiable()``."""
    from cusrl_amd.nn import module

    first = tensors[0]
    if not all(isinstance(t, torch.Tensor) for t in tensors) or not first.is_cuda or first.dim() < 1 or first.numel() < 1:
        return False
    if any(t.dtype != torch.float32 or t.device != first.device for t in tensors):
        return False
    if torch.is_autocast_enabled("cuda"):
        return False
    return not (torch.is_grad_enabled() and module._plain_linear_depth and any(t.requires_grad for t in tensors))


def gate_supported(kind: str, x, y, p, q=None, p2=None, q2=None) -> bool:
    """Do the ``cusrl_gate_*`` entries take these operands right now?  fp32 device tensors of one shape on one device, no
    autocast, and — when a gradient is asked for — a forward that is not being built inside ``double_differentiable()`` (the
    backward is once-differentiable).  Everything else keeps the reference's torch expression."""
    present = [t for t in _operands(kind, x, y, p, q, p2, q2) if t is not None]
    return _launchable(present) and all(t.shape == present[0].shape for t in present)


def glu_supported(input, dim: int = -1) -> bool:
    """Do the ``cusrl_glu_*`` entries take this input?  As :func:`gate_supported`, split along the last dimension, of even size."""
    if not isinstance(input, torch.Tensor) or input.dim() < 1 or dim not in (-1, input.dim() - 1) or input.shape[-1] % 2:
        return False
    return _launchable([input])


def _gate_expression(kind: str, x, y, p, q, p2, q2):
    """The reference's expressions (cusrl/nn/layer/gate.py:46-136), as written there."""
    p = p if p2 is None else p + p2
    if q is not None and q2 is not None:
        q = q + q2
    gate = torch.sigmoid(p)
    if kind == "input":
        return gate * x + y
    if kind == "output":
        return x + gate * y
    if kind == "highway":
        return gate * x + (1 - gate) * y
    if kind == "sigmoid_tanh":
        return x + gate * torch.tanh(q)
    if kind == "gru_reset":
        return gate * x
    return (1 - gate) * x + gate * torch.tanh(q)


def _glu_expression(kind: str, input, dim: int):
    """cusrl/nn/layer/activation.py:13-15 and :24-26."""
    x, gate = input.chunk(2, dim=dim)
    return x * (gelu(gate) if kind == "geglu" else silu(gate))


def _contiguous(*tensors):
    return tuple(None if t is None else t.contiguous() for t in tensors)  # (no copy unless a view is strided)


def _launch_gate_fwd(kind: str, x, y, p, q, p2, q2) -> torch.Tensor:
    x, y, p, q, p2, q2 = _contiguous(x, y, p, q, p2, q2)
    C = x.shape[-1]
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _checked.cusrl_gate_fwd(GATE_KINDS[kind][0], x.data_ptr(), _ptr(y), p.data_ptr(), _ptr(p2), _ptr(q), _ptr(q2), out.data_ptr(),
                            x.numel() // C, C, _stream())
    return out


def _writes_dx(kind: str) -> bool:
    return kind not in ("output", "sigmoid_tanh")


def _writes_dy(kind: str) -> bool:
    return kind in ("output", "highway")


class GateCombine(torch.autograd.Function):
    """``apply(kind, x, y, p, q, p2, q2) -> out`` on operands :func:`gate_supported` accepted (``y`` / ``q`` / ``p2`` / ``q2`` None
    where the kind takes none): one ``cusrl_gate_fwd`` launch forward, one ``cusrl_gate_bwd`` launch backward.  Only the operands
    are saved — ``x``, ``y`` and the pre-activations — and the backward recomputes the activations.  The gradient of an operand
    that enters the output as itself is the incoming gradient, handed on as it is."""

    @staticmethod
    def forward(ctx, kind, x, y, p, q, p2, q2):
        ctx.kind = kind
        # (the backward reads x only where it writes dx, y only where it writes dy: include/cusrl_hip.h's table)
        kept = (x if _writes_dx(kind) else None, y if _writes_dy(kind) else None, p, q, p2, q2)
        ctx.save_for_backward(*(t for t in kept if t is not None))
        ctx.present = tuple(t is not None for t in kept)
        return _launch_gate_fwd(kind, x, y, p, q, p2, q2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        saved = iter(ctx.saved_tensors)
        x, y, p, q, p2, q2 = (next(saved) if present else None for present in ctx.present)
        dx, dy, dp, dq = gate_backward(ctx.kind, x, y, p, q, p2, q2, dout)
        if not _writes_dx(ctx.kind):
            dx = dout
        if ctx.kind == "input":
            dy = dout
        return None, dx, dy, dp, dq, (None if p2 is None else dp), (None if q2 is None else dq)


def gate_backward(kind: str, x, y, p, q, p2, q2, dout):
    """The ``cusrl_gate_bwd`` launch by itself: ``(dx, dy, dp, dq)`` as the kind writes them (None for what it does not write;
    ``x`` / ``y`` are only read where ``dx`` / ``dy`` is written and may be None elsewhere)."""
    writes_dx, writes_dy = _writes_dx(kind), _writes_dy(kind)
    x, y, p, q, p2, q2, d = _contiguous(x if writes_dx else None, y if writes_dy else None, p, q, p2, q2, dout)
    new = lambda: torch.empty(d.shape, dtype=torch.float32, device=d.device)  # noqa: E731
    dx, dy, dp, dq = (new() if writes_dx else None), (new() if writes_dy else None), new(), (None if q is None else new())
    C = d.shape[-1]
    _checked.cusrl_gate_bwd(GATE_KINDS[kind][0], _ptr(x), _ptr(y), p.data_ptr(), _ptr(p2), _ptr(q), _ptr(q2), d.data_ptr(),
                            _ptr(dx), _ptr(dy), dp.data_ptr(), _ptr(dq), d.numel() // C, C, _stream())
    return dx, dy, dp, dq


def gate_combine(kind: str, x, y, p, q=None, p2=None, q2=None) -> torch.Tensor:
    """What a gate does with the outputs ``p`` (and ``q``) of its linear layers, bias included; ``p2`` / ``q2``: second addends
    (``p + p2``).  ``kind``: ``"input"`` ``sigmoid(p) x + y``, ``"output"`` ``x + sigmoid(p) y``, ``"highway"``
    ``g x + (1 - g) y``, ``"sigmoid_tanh"`` ``x + sigmoid(p) tanh(q)``, ``"gru_reset"`` ``sigmoid(p) x``, ``"gru_out"``
    ``(1 - z) x + z tanh(q)``.  One launch where :func:`gate_supported` says so (the forward launch alone when no gradient is
    asked for), the reference's torch expression everywhere else."""
    x, y, p, q, p2, q2 = _operands(kind, x, y, p, q, p2, q2)
    if not gate_supported(kind, x, y, p, q, p2, q2):
        return _gate_expression(kind, x, y, p, q, p2, q2)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, y, p, q, p2, q2)):
        return GateCombine.apply(kind, x, y, p, q, p2, q2)
    return _launch_gate_fwd(kind, x, y, p, q, p2, q2)


def _launch_glu_fwd(kind: str, input: torch.Tensor) -> torch.Tensor:
    input = input.contiguous()
    H = input.shape[-1] // 2
    out = torch.empty((*input.shape[:-1], H), dtype=torch.float32, device=input.device)
    _checked.cusrl_glu_fwd(GLU_KINDS[kind], input.data_ptr(), out.data_ptr(), out.numel() // H, H, _stream())
    return out


class Glu(torch.autograd.Function):
    """``apply(kind, input) -> out`` on an input :func:`glu_supported` accepted: one ``cusrl_glu_fwd`` launch forward, one
    ``cusrl_glu_bwd`` launch backward that writes both halves of the input's gradient.  Only ``input`` is saved."""

    @staticmethod
    def forward(ctx, kind, input):
        ctx.kind = kind
        ctx.save_for_backward(input)
        return _launch_glu_fwd(kind, input)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        (input,) = ctx.saved_tensors
        return None, glu_backward(ctx.kind, input, dout)


def glu_backward(kind: str, input: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    """The ``cusrl_glu_bwd`` launch by itself: the gradient of ``input`` ``[..., 2H]``, both halves."""
    input, dout = input.contiguous(), dout.contiguous()
    H = input.shape[-1] // 2
    dinput = torch.empty(input.shape, dtype=torch.float32, device=input.device)
    _checked.cusrl_glu_bwd(GLU_KINDS[kind], input.data_ptr(), dout.data_ptr(), dinput.data_ptr(), dout.numel() // H, H, _stream())
    return dinput


def glu(kind: str, input: torch.Tensor, dim: int = -1) -> torch.Tensor:
    """``a * act(b)`` for the two halves ``a, b`` of ``input`` along ``dim``; ``kind``: ``"geglu"`` (the exact GELU) or
    ``"swiglu"`` (SiLU).  One launch, the halves read in place, where :func:`glu_supported` says so (the forward launch alone
    when no gradient is asked for); the reference's torch expression everywhere else, a ``dim`` other than the last included."""
    if kind not in GLU_KINDS:
        raise ValueError(f"Unknown GLU kind '{kind}'; available kinds: {', '.join(map(repr, GLU_KINDS))}")
    if not glu_supported(input, dim):
        return _glu_expression(kind, input, dim)
    if torch.is_grad_enabled() and input.requires_grad:
        return Glu.apply(kind, input)
    return _launch_glu_fwd(kind, input)
