"""MLP pieces: ReLU-backward + bias gradient, first-layer backward, narrow heads, the one-launch inference pass
(``csrc/mlp_epilogue.hip``, ``input_layer.hip``, ``narrow_linear.hip``, ``mlp_forward.hip``)."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _f32, _observed, _ptr, _stream
from cusrl_amd.ops.gradient import DeferredColumns


def relu_backward_bias(grad_output: torch.Tensor, output: torch.Tensor | None, defer: bool = False):
    """``(grad_output * (output > 0), masked.sum(0))`` in one pass; with ``output=None`` just the column sums
    (bias gradient of a linear layer, with or without the ReLU that follows it).  ``defer``: return the column sums as
    :class:`DeferredColumns` (no finalize launch) when the layout allows; the flat gradient assembly reduces them."""
    grad_output = _f32(grad_output, "grad_output")
    H = grad_output.shape[-1]
    rows = grad_output.numel() // H
    lib = _native.lib()
    num_partials = max(int(lib.cusrl_colsum_num_partials(rows, H)), 1)
    partials = torch.empty((num_partials, H), dtype=torch.float32, device=grad_output.device)
    chunkable = H % 4 == 0 and H // 4 <= 256 and 256 % (H // 4) == 0
    defer = defer and chunkable and grad_output.data_ptr() % 16 == 0 and (output is None or output.data_ptr() % 16 == 0)
    colsum = None if defer else torch.empty(H, dtype=torch.float32, device=grad_output.device)
    if output is None:
        grad_in, out_ptr, in_ptr = grad_output, None, None
    else:
        output = _f32(output, "output")
        grad_in = torch.empty_like(grad_output)
        out_ptr, in_ptr = output.data_ptr(), grad_in.data_ptr()
    _checked.cusrl_relu_bwd_colsum(grad_output.data_ptr(), out_ptr, in_ptr, partials.data_ptr(), _ptr(colsum), rows, H, _stream())
    return grad_in, (DeferredColumns(partials, num_partials, H, 0, H) if colsum is None else colsum)


def input_layer_supported(grad_output: torch.Tensor, output: torch.Tensor | None, input: torch.Tensor, weight: torch.Tensor) -> bool:
    """Shapes and layouts ``cusrl_input_layer_bwd`` takes: fp32, contiguous, 16-byte aligned, K % 4 == 0 (<= 60), H % 64 == 0."""
    H, K = weight.shape
    tensors = [grad_output, input] + ([] if output is None else [output])
    return (bool(_native.lib().cusrl_input_layer_supported(K, H)) and input.dim() == 2 and grad_output.shape == (input.shape[0], H)
            and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tensors)
            and (output is None or output.shape == grad_output.shape) and input.shape[0] > 0)


def input_layer_backward(grad_output: torch.Tensor, output: torch.Tensor | None, input: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(dW [H, K], db [H])`` of ``y = relu(x W^T + b)`` for an input that needs no gradient, from ONE pass over ``grad_output``,
    ``output`` (the ReLU's output; None: no activation) and ``input`` (``cusrl_input_layer_bwd``); both are windows of one
    ``[H * K + H]`` row."""
    grad_output, input = _f32(grad_output, "grad_output"), _f32(input, "input")
    rows, K = input.shape
    H = grad_output.shape[-1]
    lib = _native.lib()
    dev = input.device
    width = H * K + H
    partials = torch.empty((int(lib.cusrl_input_layer_row_blocks(rows, H)), width), dtype=torch.float32, device=dev)
    grads = torch.empty(width, dtype=torch.float32, device=dev)
    _observed("cusrl_input_layer_bwd", grad_output.data_ptr(), _ptr(None if output is None else _f32(output, "output")),
            input.data_ptr(), rows, K, H, partials.data_ptr(), grads.data_ptr(),
            nbytes=lambda: rows * 4 * ((2 if output is not None else 1) * H + K) + (partials.numel() * 2 + width) * 4)
    return grads[: H * K].view(H, K), grads[H * K :]


_HEAD_PAD = 16


def narrow_linear_supported(in_features: int, out_features: int) -> bool:
    return bool(_native.lib().cusrl_narrow_linear_supported(in_features, out_features))


def narrow_linear_forward_supported(input: torch.Tensor, weight: torch.Tensor) -> bool:
    """A one-output head over a contiguous, 16-byte aligned fp32 ``[B, K]`` device matrix with K a power of two in 32..1024."""
    return (weight.dim() == 2 and weight.shape[0] == 1 and input.dim() == 2 and input.is_cuda and input.dtype == torch.float32
            and weight.dtype == torch.float32 and input.is_contiguous() and weight.is_contiguous() and input.shape[0] > 0
            and input.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0 and narrow_linear_supported(weight.shape[1], 1))


def narrow_linear_forward(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """``input @ weight.T + bias`` for a ONE-output linear layer (value head, discriminator logit) in one launch
    (``cusrl_narrow_linear_fwd``: a row dot product) instead of torch's broadcast-bias copy + skinny GEMM."""
    input, weight = _f32(input, "input"), _f32(weight, "weight")
    rows, K = input.shape
    out = torch.empty((rows, 1), dtype=torch.float32, device=input.device)
    _checked.cusrl_narrow_linear_fwd(input.data_ptr(), weight.data_ptr(), _ptr(None if bias is None else _f32(bias, "bias")),
            out.data_ptr(), rows, K, 1, _stream())
    return out


def mlp2_forward_supported(input: torch.Tensor, layers) -> bool:
    """``layers`` = ``(w1, b1, w2, b2, w3, b3)`` (``b3`` may be None) of a Linear / ReLU / Linear / ReLU / Linear stack whose shapes
    the one-launch inference pass takes (``cusrl_mlp2_forward_supported``), over a contiguous fp32 ``[B, K]`` device matrix."""
    w1, b1, w2, b2, w3, b3 = layers
    tensors = [input, w1, b1, w2, b2, w3] + ([b3] if b3 is not None else [])
    if input.dim() != 2 or input.shape[0] == 0 or any(
            (not t.is_cuda) or t.dtype != torch.float32 or (not t.is_contiguous()) or t.data_ptr() % 16 for t in tensors):
        return False
    if w1.dim() != 2 or w2.dim() != 2 or w3.dim() != 2 or w1.shape[1] != input.shape[1] or w2.shape[1] != w1.shape[0] \
            or w3.shape[1] != w2.shape[0] or b1.numel() != w1.shape[0] or b2.numel() != w2.shape[0] \
            or (b3 is not None and b3.numel() != w3.shape[0]):
        return False
    return bool(_native.lib().cusrl_mlp2_forward_supported(w1.shape[1], w1.shape[0], w2.shape[0], w3.shape[0]))


def mlp2_forward(input: torch.Tensor, layers, std: torch.Tensor | None = None, eps: torch.Tensor | None = None,
                 repeat_std: bool = True):
    """``w3 relu(w2 relu(w1 x + b1) + b2) + b3`` in ONE launch (``cusrl_mlp2_forward``), no autograd: the head's output
    ``[B, out]``; with ``std`` (``[out]`` vector) and ``eps`` (``[B, out]``) the acting path's ``(action, logp [B, 1], mean,
    repeated std or None)`` — ``action = mean + eps * std`` and its log-prob as ``normal_sample_logp`` evaluates them."""
    w1, b1, w2, b2, w3, b3 = layers
    input = _f32(input, "input")
    rows, K = input.shape
    out_features = w3.shape[0]
    out = torch.empty((rows, out_features), dtype=torch.float32, device=input.device)
    sampling = eps is not None
    action = logp = repeated = None
    if sampling:
        std, eps = _f32(std, "std"), _f32(eps, "eps")
        if std.numel() != out_features or eps.shape != out.shape:
            raise ValueError("mlp2_forward: one std per output and one eps per output element are required")
        action = torch.empty_like(out)
        logp = torch.empty((rows, 1), dtype=torch.float32, device=input.device)
        repeated = torch.empty_like(out) if repeat_std else None
    _observed(
        "cusrl_mlp2_forward", input.data_ptr(), rows, K, w1.data_ptr(), b1.data_ptr(), w1.shape[0], w2.data_ptr(),
        b2.data_ptr(), w2.shape[0], w3.data_ptr(), _ptr(b3), out_features, out.data_ptr(),
        _ptr(std) if sampling else None, _ptr(eps), _ptr(action), _ptr(logp), _ptr(repeated),
        nbytes=lambda: rows * 4 * (K + out_features * (4 if sampling else 1)) + 4 * (w1.numel() + w2.numel() + w3.numel()),
    )
    if sampling:
        return action, logp, out, repeated
    return out


def narrow_linear_backward(grad_output: torch.Tensor, input: torch.Tensor, weight: torch.Tensor,
                           need_input_grad: bool = True, relu_input: bool = False, defer: bool = False):
    """``(grad_output @ weight, grad_output.T @ input, grad_output.sum(0))`` of a linear layer with at most 16
    outputs (policy-mean / value head) in one pass over the minibatch.  With ``relu_input`` (the layer's input is a
    ReLU output) the returned grad_input is already masked by ``input > 0`` and a fourth value, its column sums
    (the bias gradient of the layer in front of the ReLU), is returned; otherwise the fourth value is None.  ``defer``:
    dW, db and the column sums come back as :class:`DeferredColumns` (no finalize launch)."""
    grad_output, input, weight = _f32(grad_output, "grad_output"), _f32(input, "input"), _f32(weight, "weight")
    O, K = weight.shape
    rows = input.shape[0]
    lib = _native.lib()
    dev = input.device
    grad_input = torch.empty_like(input) if need_input_grad else None
    width = (O + 1) * K + _HEAD_PAD
    num_partials = int(lib.cusrl_narrow_linear_num_partials(rows))
    partials = torch.empty((num_partials, width), dtype=torch.float32, device=dev)
    packed = None if defer else torch.empty(width, dtype=torch.float32, device=dev)
    _checked.cusrl_narrow_linear_bwd(grad_output.data_ptr(), input.data_ptr(), weight.data_ptr(), _ptr(grad_input),
            partials.data_ptr(), _ptr(packed), rows, K, O, int(relu_input), _stream())
    if defer:  # the three gradients stay as windows of the partial rows; cusrl_assemble_gradients sums them
        window = lambda column, numel: DeferredColumns(partials, num_partials, width, column, numel)  # noqa: E731
        return grad_input, window(0, O * K), window((O + 1) * K, O), (window(O * K, K) if relu_input else None)
    colsum = packed[O * K : (O + 1) * K] if relu_input else None
    return grad_input, packed[: O * K].view(O, K), packed[(O + 1) * K : (O + 1) * K + O], colsum
