"""The fp32-MFMA band forward without a GPU: the two symbols, the shapes the library takes, and what CPU tensors take."""

import torch

from cusrl_amd import _native, ops


def test_symbols_are_bound_and_the_abi_stays_7():
    assert {"cusrl_band_sdpa_fwd_mfma", "cusrl_band_sdpa_fwd_mfma_supported"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert _native._PROTOTYPES["cusrl_band_sdpa_fwd_mfma"] == _native._PROTOTYPES["cusrl_band_sdpa_fwd"]
    supported = _native.lib().cusrl_band_sdpa_fwd_mfma_supported  # (Lq, W, D)
    assert supported(2, 1, 4) and supported(33, 17, 128) and supported(5, 7, 12)
    assert not any(supported(*sizes) for sizes in ((1, 7, 8), (5, 7, 6), (5, 7, 2), (5, 7, 132), (5, 0, 8)))


def test_cpu_tensors_take_the_dense_mask_as_before():
    torch.manual_seed(5)
    q, k, v = torch.randn(2, 5, 3, 8), torch.randn(2, 9, 3, 8), torch.randn(2, 9, 3, 8)
    valid = torch.arange(9).expand(2, 9) % 4 != 3
    assert not ops.band_sdpa_mfma_supported(q, k, v, 4, valid)
    before = dict(_native.launch_counts)
    want = ops.sdpa(q, k, v, attn_mask=ops.band_mask(q, 4, valid))
    assert torch.equal(ops.band_sdpa(q, k, v, 4, valid, matrix_core=True), want)
    with ops.matrix_core_attention():
        assert torch.equal(ops.band_sdpa(q, k, v, 4, valid), want)
    assert _native.launch_counts == before
