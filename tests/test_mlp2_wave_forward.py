"""The host side of ``cusrl_mlp2_wave_forward``: its two symbols in the binding, at an unchanged ABI version."""

from __future__ import annotations


def test_the_binding_declares_both_symbols_at_abi_7():
    from cusrl_amd import _native

    assert {"cusrl_mlp2_wave_forward", "cusrl_mlp2_wave_forward_supported"} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.ABI_VERSION == 7
