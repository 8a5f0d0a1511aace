"""The host side of ``cusrl_mlp3_forward``: its two symbols in the binding, what ``Mlp.inference_stack3`` describes and refuses,
and the conditions on the integer stacks (tests/_mlp3_forward.py) that entitle the device test to ``torch.equal``.  If a
condition fails, the draw is to be changed, not the condition."""

from __future__ import annotations

import pytest
import torch
from torch import nn

import _mlp3_forward as M


def test_the_binding_declares_both_symbols_at_abi_7():
    from cusrl_amd import _native

    assert {"cusrl_mlp3_forward", "cusrl_mlp3_forward_supported"} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.ABI_VERSION == 7


def test_inference_stack3_describes_three_activated_layers_and_nothing_else():
    from cusrl_amd import preset
    from cusrl_amd.nn.module import Mlp

    mlp = Mlp(48, (512, 256, 128), activation_fn="ELU", ends_with_activation=True)
    *weights, name, alpha = mlp.inference_stack3()
    assert (name, alpha) == ("ELU", 1.0) and [tuple(w.shape) for w in weights] == [(512, 48), (512,), (256, 512), (256,), (128, 256), (128,)]
    assert all(w is p for w, p in zip(weights, mlp.parameters()))
    assert Mlp(48, (128, 128, 128), activation_fn="Tanh", ends_with_activation=True).inference_stack3()[6:] == ("Tanh", 1.0)
    assert mlp.inference_stack() is None
    for other in (Mlp(48, (512, 256, 128), activation_fn="ELU", ends_with_activation=True, dropout=0.1),
                  Mlp(48, (512, 256, 128), activation_fn="ELU"),
                  Mlp(48, (256, 128), activation_fn="ELU", ends_with_activation=True),
                  Mlp(48, (512, 256, 128), activation_fn="GELU", ends_with_activation=True)):
        assert other.inference_stack3() is None
    # the preset's two-layer ReLU backbone: what inference_stack returns is unchanged
    backbone = preset.PpoAgentFactory().to_underlying().actor_factory.backbone_factory(48, None)
    layers = backbone.layers
    assert [type(m) for m in layers[1::2]] == [nn.ReLU, nn.ReLU] and backbone.inference_stack3() is None
    stack = backbone.inference_stack()
    assert len(stack) == 4 and all(a is b for a, b in zip(stack, (layers[0].weight, layers[0].bias, layers[2].weight, layers[2].bias)))


@pytest.mark.parametrize("widths", M.TRIPLES, ids=str)
@pytest.mark.parametrize("K", M.EXACT_KS)
def test_integer_stacks_are_exact_in_fp32_and_cut_both_ways(K, widths):
    x, layers = M.integer_stack(K, widths)
    for bias4 in (True, False):
        used = layers if bias4 else (*layers[:7], None)
        out, mag, hidden = M.integer_reference(K, widths, bias4)
        print(f"{K}->{widths}: largest magnitude {float(mag.max()):.3g}, live {[round(float((h > 0).double().mean()), 2) for h in hidden]}")
        assert float(mag.max()) < 2 ** 24
        assert torch.equal(M.library_chain(x, used, "ReLU").double(), out), "torch's fp32 chain on the host differs from float64"
        assert all(0.2 <= float((h > 0).double().mean()) <= 0.8 for h in hidden)
