"""The one-launch recurrent time step (csrc/recurrent_step.hip) without a GPU: its symbols are bound, its switch is a context."""

from __future__ import annotations

import pytest

from cusrl_amd import _native, ops

SYMBOLS = {"cusrl_gru_step_forward", "cusrl_gru_step_forward_supported", "cusrl_lstm_step_forward", "cusrl_lstm_step_forward_supported"}


def test_the_four_symbols_are_bound_and_the_abi_stays_7():
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert all(hasattr(_native.lib(), symbol) for symbol in SYMBOLS)


def test_fused_recurrent_step_nests_and_restores_its_state():
    assert not ops.fused_recurrent_step_enabled()
    with ops.fused_recurrent_step():
        assert ops.fused_recurrent_step_enabled()
        with ops.fused_recurrent_step(False):
            assert not ops.fused_recurrent_step_enabled()
        assert ops.fused_recurrent_step_enabled()
        with pytest.raises(KeyError), ops.fused_recurrent_step(False):
            raise KeyError("inside")
        assert ops.fused_recurrent_step_enabled()
    assert not ops.fused_recurrent_step_enabled()
