"""The fp32-MFMA band backward without a GPU: the two symbols, the shapes the library takes, and what CPU tensors take."""

import torch

from cusrl_amd import _native, ops


def test_symbols_are_bound_and_the_abi_stays_7():
    assert {"cusrl_band_sdpa_bwd_mfma", "cusrl_band_sdpa_bwd_mfma_supported"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION == 7
    assert _native._PROTOTYPES["cusrl_band_sdpa_bwd_mfma"] == _native._PROTOTYPES["cusrl_band_sdpa_bwd"]
    supported = _native.lib().cusrl_band_sdpa_bwd_mfma_supported  # (Lq, W, D)
    assert supported(2, 1, 4) and supported(33, 17, 128) and supported(5, 7, 12)
    assert not any(supported(*sizes) for sizes in ((1, 7, 8), (5, 7, 6), (5, 7, 2), (5, 7, 132), (5, 0, 8)))


def test_cpu_tensors_take_the_dense_mask_as_before():
    torch.manual_seed(5)
    q, k, v = (torch.randn(2, L, 3, 8, requires_grad=True) for L in (5, 9, 9))
    valid = torch.arange(9).expand(2, 9) % 4 != 3
    assert not ops.band_sdpa_bwd_mfma_supported(q, k, v, 4, valid)
    before = dict(_native.launch_counts)

    def run(**kwargs):
        out = ops.band_sdpa(q, k, v, 4, valid, **kwargs)
        return [out.detach(), *torch.autograd.grad(out.sum(), (q, k, v))]

    want = [(dense := ops.sdpa(q, k, v, attn_mask=ops.band_mask(q, 4, valid))).detach(), *torch.autograd.grad(dense.sum(), (q, k, v))]
    assert all(torch.equal(a, b) for a, b in zip(run(matrix_core_backward=True), want))
    with ops.matrix_core_attention(backward=True):
        assert all(torch.equal(a, b) for a, b in zip(run(), want))
    assert _native.launch_counts == before
