"""The one-launch attention step (csrc/attention_step.hip) without a GPU: its symbols are bound, its ``_supported`` twin states
the shapes, its switch is a context, and nothing outside a no-grad single step without RoPE inside that context reaches it."""

from __future__ import annotations

import pytest
import torch

from cusrl_amd import _native, nn, ops

SYMBOLS = {"cusrl_attn_step_forward", "cusrl_attn_step_forward_supported"}


def test_the_two_symbols_are_bound_and_the_abi_stays_7():
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7 and all(hasattr(_native.lib(), s) for s in SYMBOLS)


def _operands(N=3, H=4, W=5, C=8):
    out = (torch.empty(N, H, C), torch.empty(N, W, C), torch.empty(N, W, dtype=torch.bool))
    return [torch.zeros(N, H, C), torch.zeros(N, C), torch.zeros(N, W, C), torch.ones(N, W, dtype=torch.bool)], out


@pytest.mark.parametrize("sizes", (dict(H=17), dict(C=6), dict(C=132), dict(W=0)))
def test_the_supported_twin_refuses_other_sizes(sizes):
    good, out = _operands()
    assert ops.attention_step_supported(*good, out=out) and ops.attention_step_supported(*good)
    assert ops.attention_step_supported(good[0], good[1], None, None, window=5)
    bad, out = _operands(**sizes)
    assert not ops.attention_step_supported(*bad, out=out)


def test_the_supported_twin_refuses_a_misaligned_pointer_and_an_aliased_roll():
    (qf, x, cache, mask), out = _operands()
    shifted = torch.zeros(x.numel() + 1)[1:].view_as(x)   # 4 bytes off a 16-byte boundary
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    assert not ops.attention_step_supported(qf, shifted, cache, mask, out=out)
    assert not ops.attention_step_supported(qf, x, cache, mask, out=(out[0], cache, out[2]))
    assert not ops.attention_step_supported(qf, x, cache, mask, out=(out[0], out[1], mask))
    assert not ops.attention_step_supported(qf, x, cache, mask, out=(qf, out[1], out[2]))


def test_fused_attention_step_nests_and_restores_its_state():
    assert not ops.fused_attention_step_enabled()
    with ops.fused_attention_step():
        assert ops.fused_attention_step_enabled()
        with ops.fused_attention_step(False):
            assert not ops.fused_attention_step_enabled()
        assert ops.fused_attention_step_enabled()
        with pytest.raises(KeyError), ops.fused_attention_step(False):
            raise KeyError("inside")
        assert ops.fused_attention_step_enabled()
    assert not ops.fused_attention_step_enabled()


def test_the_module_stays_on_its_own_path_everywhere_else():
    torch.manual_seed(0)
    plain, rope = (nn.CausalMultiheadSelfAttention(8, 2, 4, rope_base=base) for base in (None, 100.0))
    step, two = torch.randn(3, 8), torch.randn(2, 3, 8)
    before = _native.launch_counts.get("cusrl_attn_step_forward", 0)
    with torch.no_grad():
        outside = plain(step)[0]
    with ops.fused_attention_step():
        assert torch.equal(plain(step)[0], outside)           # grad enabled
        with torch.no_grad():
            rope(step), plain(two)                            # RoPE, L = 2
    assert _native.launch_counts.get("cusrl_attn_step_forward", 0) == before
