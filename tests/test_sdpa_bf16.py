"""The bf16 attention forward without a GPU: symbols, supported set, CPU tensors, refusals on placeholder pointers (never read)."""

import pytest
import torch

from cusrl_amd import _native, ops


def test_symbols_are_bound_and_the_abi_stays_7():
    assert {"cusrl_sdpa_fwd_bf16", "cusrl_sdpa_fwd_bf16_supported"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert len(_native._PROTOTYPES["cusrl_sdpa_fwd_bf16"][1]) == len(_native._PROTOTYPES["cusrl_sdpa_fwd_mfma"][1])
    supported = _native.lib().cusrl_sdpa_fwd_bf16_supported
    assert {D: bool(supported(3, 5, D)) for D in (4, 8, 12, 24, 128, 136)} == {4: False, 8: True, 12: False, 24: True, 128: True, 136: False}
    assert supported(1, 1, 8) and not supported(0, 3, 8) and not supported(3, 0, 8)


def test_cpu_bf16_tensors_take_the_torch_expression():
    torch.manual_seed(3)
    q, k, v = (torch.randn(2, L, 3, 8).bfloat16() for L in (5, 7, 7))
    assert not ops.sdpa_bf16_supported(q, k, v)
    sdpa, before = torch.nn.functional.scaled_dot_product_attention, dict(_native.launch_counts)
    assert torch.equal(ops.sdpa(q, k, v, matrix_core=True), sdpa(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2))
    assert _native.launch_counts == before


@pytest.mark.parametrize("change,status", [({"out": 0}, -1), ({"D": 12}, -3), ({"q": 4096 + 8}, -3), ({"stride_l": 3 * 8 + 4}, -3)],
                         ids=["null-out", "D-12", "misaligned-base", "stride-not-a-multiple-of-8"])
def test_refusals_come_before_any_launch(change, status):
    a = dict({"q": 4096, "out": 8192, "D": 8, "stride_l": 3 * 8}, **change)
    N, H, Lq, Lk, D = 2, 3, 5, 7, a["D"]
    got = _native.lib().cusrl_sdpa_fwd_bf16(a["q"], Lq * a["stride_l"], a["stride_l"], 4096, Lk * H * D, H * D, 4096, Lk * H * D, H * D, None,
                                            None, 0, 0, 0, 0, 0, 1.0, a["out"], 4096, N, H, Lq, Lk, D, None)
    assert got == status
