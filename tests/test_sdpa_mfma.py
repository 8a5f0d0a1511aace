"""The fp32-MFMA attention forward without a GPU: the two symbols, what CPU tensors take, and the context manager's state."""

import pytest
import torch

from cusrl_amd import _native, ops
from cusrl_amd.ops import attention


def _torch_expression(q, k, v, **kwargs):
    sdpa = torch.nn.functional.scaled_dot_product_attention
    return sdpa(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), **kwargs).transpose(1, 2)


def test_symbols_are_bound_and_the_abi_stays_7():
    assert {"cusrl_sdpa_fwd_mfma", "cusrl_sdpa_fwd_mfma_supported"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert _native._PROTOTYPES["cusrl_sdpa_fwd_mfma"] == _native._PROTOTYPES["cusrl_sdpa_fwd"]
    supported = _native.lib().cusrl_sdpa_fwd_mfma_supported
    assert supported(1, 1, 4) and supported(65, 33, 128) and supported(3, 3, 12)
    assert not any(supported(*sizes) for sizes in ((3, 3, 6), (3, 3, 2), (3, 3, 132), (0, 3, 8), (3, 0, 8)))


def test_cpu_tensors_take_the_torch_expression():
    torch.manual_seed(3)
    q, k, v = torch.randn(2, 5, 3, 8), torch.randn(2, 7, 3, 8), torch.randn(2, 7, 3, 8)
    assert not ops.sdpa_mfma_supported(q, k, v)
    before = dict(_native.launch_counts)
    assert torch.equal(ops.sdpa(q, k, v, matrix_core=True), _torch_expression(q, k, v))
    with ops.matrix_core_attention():
        assert torch.equal(ops.sdpa(q, k[:, :5], v[:, :5], is_causal=True), _torch_expression(q, k[:, :5], v[:, :5], is_causal=True))
    assert _native.launch_counts == before


def test_the_context_restores_the_previous_state():
    state = lambda: getattr(attention._matrix_core, "enabled", False)  # noqa: E731
    assert state() is False
    with ops.matrix_core_attention():
        assert state() is True
        with ops.matrix_core_attention(False):
            assert state() is False
        assert state() is True
        with pytest.raises(KeyError), ops.matrix_core_attention(False):
            raise KeyError("inside")
        assert state() is True
    assert state() is False
