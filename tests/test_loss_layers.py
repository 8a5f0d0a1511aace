"""``NormalNllLoss`` and ``L2RegularizationLoss`` without a GPU: the exports, the constructor's errors in the reference's words,
the host (torch) expression against every recorded case of golden ``loss_layers.npz``, and the C ABI of
``cusrl_normal_nll_fwd_bwd`` as far as it goes without a launch.  Bounds: 1e-5 relative for a loss, 1e-5 of the largest entry
for a gradient — the project's standing ones."""

from __future__ import annotations

import math

import pytest
import torch

from _loss_layers import CASES, EPS, FORMS, GOLDEN, MODES, check_loss, expected, parse, run_case


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.mark.parametrize("name", ["NormalNllLoss", "L2RegularizationLoss", "GradientPenaltyLoss"])
def test_the_layers_are_exported(cusrl, name):
    import cusrl_amd.nn.loss as loss_module

    assert getattr(cusrl, name) is getattr(cusrl.nn, name)
    assert issubclass(getattr(cusrl, name), torch.nn.Module)
    assert name in cusrl.__all__ and name in cusrl.nn.__all__
    if name == "GradientPenaltyLoss":
        assert cusrl.nn.GradientPenaltyLoss is cusrl.hook.auxiliary.amp.GradientPenaltyLoss  # where it already lived
    else:
        assert getattr(loss_module, name) is getattr(cusrl, name) and name in loss_module.__all__


def test_constructor_attributes_and_errors_are_the_references(cusrl):
    layer = cusrl.nn.NormalNllLoss()
    assert (layer.mode, layer.full, layer.eps, layer.reduction) == ("log_var", False, 1e-6, "mean")
    assert layer.sqrt_eps == math.sqrt(1e-6) and layer.log_eps == math.log(1e-6)
    layer = cusrl.nn.NormalNllLoss(mode="std", full=True, eps=0.25, reduction="none")
    assert (layer.mode, layer.full, layer.eps, layer.sqrt_eps, layer.log_eps, layer.reduction) == (
        "std", True, 0.25, 0.5, math.log(0.25), "none")
    with pytest.raises(TypeError):
        cusrl.nn.NormalNllLoss("var")  # keyword-only, like the reference's
    for eps in (0.0, -1e-3):
        with pytest.raises(ValueError, match="^'eps' must be greater than zero$"):
            cusrl.nn.NormalNllLoss(eps=eps)
    with pytest.raises(ValueError, match="^Unsupported mode 'sigma'; expected one of 'log_var', 'log_std', 'var', or 'std'$"):
        cusrl.nn.NormalNllLoss(mode="sigma")
    assert cusrl.nn.L2RegularizationLoss().reduction == "mean" and cusrl.nn.L2RegularizationLoss("sum").reduction == "sum"


def test_the_golden_covers_what_it_is_meant_to():
    reduced = {parse(case)[1:] for case in CASES if parse(case)[0] == "37x7"}
    assert {(mode, full, reduction) for mode in MODES for full in (False, True) for reduction in ("mean", "sum")} <= reduced
    assert {mode for _, mode, _, reduction in map(parse, CASES) if reduction == "none"} == set(MODES)
    assert {"1x1", "37x7", "5x12", "6x4", "3x5x8", "1031x17", "9x6@leaf"} == {parse(case)[0] for case in CASES}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_host_expression_matches_the_reference(cusrl, case, form, gradient_parity, monkeypatch):
    """On CPU tensors the layer evaluates the reference's expression — in any process: it asks for no ``host_form`` opt-in."""
    monkeypatch.delenv("CUSRL_HOST_FORMS", raising=False)
    target_grad = parse(case)[0] != "1031x17"  # (the large shape records no d_target)
    loss, grads = run_case(cusrl, case, form, target_grad=target_grad)
    check_loss(loss, expected(case, "loss"), gradient_parity, f"loss_layers.host.unreduced[{case},{form}]")
    for name, gradient in grads.items():
        gradient_parity(f"loss_layers.host.{name}[{case},{form}]", gradient.numpy(), expected(case, name), 1e-5)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_l2_host_expression_matches_the_reference(cusrl, reduction, gradient_parity, monkeypatch):
    monkeypatch.delenv("CUSRL_HOST_FORMS", raising=False)
    x = torch.from_numpy(GOLDEN["l2_input"]).requires_grad_()
    loss = cusrl.nn.L2RegularizationLoss(reduction=reduction)(x)
    loss.backward(torch.ones_like(loss))
    check_loss(loss, GOLDEN[f"l2_{reduction}_loss"], gradient_parity, "loss_layers.host.l2_unreduced")
    gradient_parity(f"loss_layers.host.l2[{reduction}]", x.grad.numpy(), GOLDEN[f"l2_{reduction}_d_input"], 1e-5)


def test_an_odd_chunked_width_fails_as_the_references_does(cusrl):
    with pytest.raises(RuntimeError):  # chunk gives a 3-wide mean and a 2-wide parameter: they do not broadcast
        cusrl.nn.NormalNllLoss()(torch.randn(4, 5), torch.randn(4, 3))


def test_the_binding_exports_the_kernel_and_its_sizing_helper(cusrl):
    from cusrl_amd import _native, ops

    assert {"cusrl_normal_nll_fwd_bwd", "cusrl_normal_nll_num_partials"} <= set(_native.EXPORTED_SYMBOLS)
    assert callable(ops.normal_nll_fwd_bwd) and _native.ABI_VERSION == 7
    lib = _native.lib()
    # the launch rule of cusrl_mse_loss_num_partials on rows * K elements: one self-finalising block up to 16 K elements
    assert lib.cusrl_normal_nll_num_partials(1, 1) == lib.cusrl_normal_nll_num_partials(37, 7) == 1
    assert lib.cusrl_normal_nll_num_partials(1024, 16) == 1 and lib.cusrl_normal_nll_num_partials(16385, 1) == 9
    assert lib.cusrl_normal_nll_num_partials(1031, 17) == lib.cusrl_mse_loss_num_partials(1031 * 17) == 9
    assert lib.cusrl_normal_nll_num_partials(70000, 31) == 1024
    assert lib.cusrl_normal_nll_num_partials(0, 4) == lib.cusrl_normal_nll_num_partials(4, 0) == 0
    assert lib.cusrl_normal_nll_num_partials(1 << 30, 4) == 0  # nothing beyond a 32-bit element index


def test_bad_arguments_are_refused_before_any_launch(cusrl):
    from cusrl_amd import _native

    lib = _native.lib()
    invalid, unsupported = _native._CONSTANTS["E_INVALID"], _native._CONSTANTS["E_UNSUPPORTED"]
    p = 0x1000  # a non-null placeholder: these calls return before touching it

    def call(**kw):
        pointers = {name: kw.get(name, p) for name in ("mean", "dist", "target", "loss", "d_mean", "d_dist", "partials")}
        K = kw.get("K", 4)
        pitch = {name: kw.get(name, K) for name in ("mean_pitch", "dist_pitch", "target_pitch", "grad_pitch")}
        return lib.cusrl_normal_nll_fwd_bwd(
            pointers["mean"], pitch["mean_pitch"], pointers["dist"], pitch["dist_pitch"], pointers["target"], pitch["target_pitch"],
            kw.get("rows", 2), K, kw.get("mode", 0), kw.get("full", 0), math.log(EPS), kw.get("reduction", 1), pointers["loss"],
            pointers["d_mean"], pointers["d_dist"], pitch["grad_pitch"], pointers["partials"], None)

    for name in ("mean", "dist", "target", "loss", "d_mean", "d_dist", "partials"):
        assert call(**{name: None}) == invalid, name
    assert call(rows=0) == invalid and call(K=0) == invalid and call(rows=-3) == invalid
    for name in ("mean_pitch", "dist_pitch", "target_pitch", "grad_pitch"):
        assert call(**{name: 3}) == invalid, name  # a pitch below K
    assert call(mode=-1) == invalid and call(mode=4) == invalid
    assert call(reduction=0) == invalid and call(reduction=3) == invalid
    assert call(full=2) == invalid
    assert call(rows=1 << 30) == unsupported
    assert invalid < 0 and unsupported < 0


def test_the_binding_refuses_host_tensors(cusrl):
    from cusrl_amd import ops

    with pytest.raises(RuntimeError, match="lives on cpu"):
        ops.normal_nll_fwd_bwd(torch.randn(4, 6), None, torch.randn(4, 3), "log_var", False, 1e-6, "mean")
    with pytest.raises(ValueError, match="reduces by 'mean' or 'sum'"):
        ops.normal_nll_fwd_bwd(torch.randn(4, 6), None, torch.randn(4, 3), "log_var", False, 1e-6, "none")
    assert ops.normal_nll_bound("log_std", 1e-2) == math.log(1e-2) / 2 and ops.normal_nll_bound("std", 0.25) == 0.5
