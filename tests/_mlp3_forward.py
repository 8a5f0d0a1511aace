"""Shared by tests/test_mlp3_forward.py (CPU) and tests/test_mlp3_forward_gpu.py: the integer stacks on which every fp32
summation order of ``cusrl_mlp3_forward`` gives the float64 result, and the float64 reference of a three-layer stack.

The draw (seed 1, 37 rows, 16 outputs): x and every bias are integers in [-2, 2], every weight is in {-1, 0, 1}; W1 and W4 are
dense, W2 and W3 thinned to a kept share of 1/8 and 1/4, which keeps the accumulated magnitude under 2^24.  Fewer rows are the
first rows, a narrower head the first rows of W4: one float64 evaluation per (K, widths) serves them all."""

from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

TRIPLES = ((512, 256, 128), (256, 128, 64), (128, 128, 128))
EXACT_KS = (4, 20, 64)      # one live quad, a partial last k-block, the full K
EXACT_ROWS = (1, 17, 37)
EXACT_OUTS = (1, 5, 16)
UNSUPPORTED = -3            # CUSRL_E_UNSUPPORTED
ACT = {"ReLU": torch.relu, "ELU": F.elu, "Tanh": torch.tanh}


def reference(x, layers, activation):
    """float64 ``(out, mag, hidden)``: the stack, the magnitude its fp32 sums accumulate, the three hidden layers."""
    act = ACT[activation]
    h, mag, hidden = x.double().cpu(), x.double().cpu().abs(), []
    for weight, bias in zip(layers[0::2], layers[1::2]):
        weight = weight.double().cpu()
        h, mag = h @ weight.T, mag @ weight.abs().T
        if bias is not None:
            h, mag = h + bias.double().cpu(), mag + bias.double().cpu().abs()
        if len(hidden) < 3:
            h = act(h)
            hidden.append(h)
    return h, mag, hidden


def library_chain(x, layers, activation):
    """torch's own fp32 chain (F.linear + activation) on the device of its operands."""
    for weight, bias in zip(layers[0:6:2], layers[1:6:2]):
        x = ACT[activation](F.linear(x, weight, bias))
    return F.linear(x, layers[6], layers[7])


@functools.lru_cache(maxsize=None)
def integer_stack(K, widths):
    """``(x [37, K], (w1, b1, ..., w4 [16, H3], b4 [16]))`` as fp32 CPU tensors of small integers (nobody writes to them)."""
    g = torch.Generator().manual_seed(1)
    ints = lambda low, high, *shape: torch.randint(low, high + 1, shape, generator=g).float()  # noqa: E731
    thinned = lambda w, keep: w * (torch.rand(w.shape, generator=g) < keep)  # noqa: E731
    H1, H2, H3 = widths
    x = ints(-2, 2, EXACT_ROWS[-1], K)
    return x, (ints(-1, 1, H1, K), ints(-2, 2, H1), thinned(ints(-1, 1, H2, H1), 1 / 8), ints(-2, 2, H2),
               thinned(ints(-1, 1, H3, H2), 1 / 4), ints(-2, 2, H3), ints(-1, 1, 16, H3), ints(-2, 2, 16))


@functools.lru_cache(maxsize=None)
def integer_reference(K, widths, bias4=True):
    x, layers = integer_stack(K, widths)
    return reference(x, layers if bias4 else (*layers[:7], None), "ReLU")


def integer_case(K, widths, rows, A, bias4=True):
    """``(x, layers, float64 expectation)`` of the first ``rows`` rows and the first ``A`` outputs."""
    x, layers = integer_stack(K, widths)
    layers = (*layers[:6], layers[6][:A].contiguous(), layers[7][:A].contiguous() if bias4 else None)
    return x[:rows].contiguous(), layers, integer_reference(K, widths, bias4)[0][:rows, :A].contiguous()
