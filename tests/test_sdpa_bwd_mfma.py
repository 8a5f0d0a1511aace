"""The fp32-MFMA attention backward without a GPU: the two symbols, what CPU tensors take, and the context manager's two fields."""

import pytest
import torch

from cusrl_amd import _native, ops
from cusrl_amd.ops import attention


def test_symbols_are_bound_the_abi_stays_7_and_the_truth_table_is_the_forwards():
    assert {"cusrl_sdpa_bwd_mfma", "cusrl_sdpa_bwd_mfma_supported"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert _native._PROTOTYPES["cusrl_sdpa_bwd_mfma"] == _native._PROTOTYPES["cusrl_sdpa_bwd"]
    lib, yes = _native.lib(), ((1, 1, 4), (65, 33, 128), (3, 3, 12))
    for sizes in (*yes, (3, 3, 6), (3, 3, 2), (3, 3, 132), (0, 3, 8), (3, 0, 8)):
        assert bool(lib.cusrl_sdpa_bwd_mfma_supported(*sizes)) == bool(lib.cusrl_sdpa_fwd_mfma_supported(*sizes)) == (sizes in yes), sizes


def test_cpu_tensors_take_the_torch_expression():
    torch.manual_seed(3)
    q, k, v = (torch.randn(2, 5, 3, 8, requires_grad=True) for _ in range(3))
    assert not ops.sdpa_bwd_mfma_supported(q, k, v)
    before = dict(_native.launch_counts)
    want = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True).transpose(1, 2)
    with ops.matrix_core_attention(backward=True):
        for got in (ops.sdpa(q, k, v, is_causal=True, matrix_core_backward=True), ops.sdpa(q, k, v, is_causal=True)):
            assert torch.equal(got, want)
            assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(got.sum(), (q, k, v)), torch.autograd.grad(want.sum(), (q, k, v), retain_graph=True)))
    assert _native.launch_counts == before


def test_the_context_restores_both_fields():
    state = lambda: (getattr(attention._matrix_core, "enabled", False), getattr(attention._matrix_core, "backward", False))  # noqa: E731
    assert state() == (False, False)
    with ops.matrix_core_attention(backward=True):
        assert state() == (True, True)
        with ops.matrix_core_attention(False):  # (backward falls to its default inside)
            assert state() == (False, False)
        with pytest.raises(KeyError), ops.matrix_core_attention(False, backward=True):
            assert state() == (False, True)
            raise KeyError("inside")
        assert state() == (True, True)
    assert state() == (False, False)
