"""``ActionSmoothnessLoss`` without a GPU: the exports, the hook's torch expression against every recorded case of golden
``smoothness.npz`` (the reference's ``objective`` on CPU), the reference's error messages, the mutable weights, the hook's place
in a factory, the closed form in float64 against the same recordings, and the C ABI of ``cusrl_action_smoothness_fwd_bwd`` as
far as it goes without a launch.  Bounds: 1e-5 relative for a loss, 1e-5 of the largest entry for a gradient — the project's
standing ones."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _smoothness import (CASES, EMPTY_INPUTS, GOLDEN, INPUTS, KEY_1ST, KEY_2ND, case_inputs, case_weights, check_case,
                         closed_form_f64, expected, make_hook, parse, run_case)

KERNEL = "cusrl_action_smoothness_fwd_bwd"


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def test_the_hook_is_exported(cusrl):
    from cusrl_amd.hook.auxiliary import smoothness

    assert cusrl.hook.ActionSmoothnessLoss is cusrl.hook.auxiliary.ActionSmoothnessLoss is smoothness.ActionSmoothnessLoss
    assert "ActionSmoothnessLoss" in cusrl.hook.__all__ and "ActionSmoothnessLoss" in cusrl.hook.auxiliary.__all__
    assert issubclass(cusrl.hook.ActionSmoothnessLoss, cusrl.Hook)
    hook = cusrl.hook.ActionSmoothnessLoss()
    assert hook.name == "action_smoothness_loss"
    assert (hook.weight_1st_order, hook.weight_2nd_order) == (None, None)
    assert hook._mutable == {"weight_1st_order", "weight_2nd_order"}
    hook = cusrl.hook.ActionSmoothnessLoss(0.5, [0.1, 0.2])
    assert (hook.weight_1st_order, hook.weight_2nd_order) == (0.5, [0.1, 0.2])


def test_the_golden_covers_what_it_is_meant_to():
    assert INPUTS == ["T3,B1,A1", "T3,B2,A1@done_at_0_0", "T3,B2,A1@all_done_at_0", "T5,B3,A2", "T8,B300,A7", "T24,B37,A12",
                      "T6,B4,A3@constant_column"]
    assert EMPTY_INPUTS == {"T3,B2,A1@all_done_at_0"}
    assert set(CASES) == {f"{name}|{terms}|{form}" for name in INPUTS for terms in ("1", "2", "12")
                          for form in ("scalar", "sequence")}
    for case in CASES:
        name = parse(case)[0]
        n1, n2 = int(expected(case, "n1")), int(expected(case, "n2"))
        assert n1 > 0 and (n2 > 0) == (name not in EMPTY_INPUTS), case
    done = GOLDEN["in/T5,B3,A2/done"][:, :, 0]
    assert not done[:, 0].any() and done[:, 1].tolist() == [True, True, False, False, False]
    assert done[:, 2].tolist() == [False, False, False, False, True]
    constant = GOLDEN["in/T6,B4,A3@constant_column/mean"][:, :, 1]
    assert (constant == constant[0]).all()
    assert int(GOLDEN["in/T8,B300,A7/mean"][0].size) % 64 != 0 and GOLDEN["in/T8,B300,A7/mean"][0].size > 256


@pytest.mark.parametrize("case", CASES)
def test_host_expression_matches_the_reference(cusrl, case, gradient_parity):
    losses, d_mean = run_case(cusrl, case)
    check_case(case, losses, d_mean, None, gradient_parity, f"host,{case}")


@pytest.mark.parametrize("case", CASES)
def test_the_closed_form_in_float64_matches_the_reference(case, gradient_parity):
    """Pins the formula, not only the recording: validity from shifted ``done`` flags, the divisor ``n_k A``, ``sign(0) = 0``."""
    mean, done = case_inputs(case)
    w1, w2 = case_weights(case)
    result = closed_form_f64(mean.numpy(), done.numpy(), w1, w2)
    losses = {key: result[name] for key, name in ((KEY_1ST, "loss1"), (KEY_2ND, "loss2")) if name in result}
    check_case(case, losses, result["d_mean"], (result["n1"], result["n2"]), gradient_parity, f"f64,{case}")


def test_a_constant_column_gets_no_gradient(cusrl):
    case = "T6,B4,A3@constant_column|12|sequence"
    assert not expected(case, "d_mean")[:, :, 1].any()  # sign(0) = 0 in the reference
    _, d_mean = run_case(cusrl, case)
    assert not d_mean[:, :, 1].any() and d_mean[:, :, 0].any()


def test_errors_are_the_references(cusrl):
    hook = make_hook(cusrl, 0.1, 0.1)
    with pytest.raises(ValueError, match=r"^Expected batch to be temporal\.$"):
        hook.objective({}, {"curr_action_dist": {"mean": torch.randn(6, 3)}, "done": torch.zeros(6, 1, dtype=torch.bool)})
    for steps in (1, 2):
        with pytest.raises(ValueError, match=rf"^Expected sequences to have at least 3 time steps, but got {steps}\.$"):
            hook.objective({}, {"curr_action_dist": {"mean": torch.randn(steps, 4, 3)},
                                "done": torch.zeros(steps, 4, 1, dtype=torch.bool)})
    # the checks come first, whatever the weights are
    with pytest.raises(ValueError, match="temporal"):
        make_hook(cusrl, None, None).objective({}, {"curr_action_dist": {"mean": torch.randn(6, 3)}, "done": None})


def test_no_weights_give_no_terms(cusrl):
    mean, done = case_inputs("T5,B3,A2|12|scalar")
    assert make_hook(cusrl, None, None).objective({}, {"curr_action_dist": {"mean": mean}, "done": done}) == {}


def test_update_attribute_changes_the_next_result(cusrl):
    case = "T5,B3,A2|12|scalar"
    mean, done = case_inputs(case)
    batch = {"curr_action_dist": {"mean": mean}, "done": done}
    hook = make_hook(cusrl, *case_weights(case))
    first = hook.objective({}, batch)
    hook.update_attribute("weight_1st_order", 3 * hook.weight_1st_order)
    second = hook.objective({}, batch)
    np.testing.assert_allclose(float(second[KEY_1ST]), 3 * float(first[KEY_1ST]), rtol=1e-6)
    assert float(second[KEY_2ND]) == float(first[KEY_2ND])
    hook.update_attribute("weight_2nd_order", [0.5, 0.25])
    per_column = hook.objective({}, batch)
    w2 = case_weights(case)[1]
    reference = closed_form_f64(mean.numpy(), done.numpy(), None, [0.5, 0.25])["loss2"]
    np.testing.assert_allclose(float(per_column[KEY_2ND]), reference, rtol=1e-5)
    assert w2 != [0.5, 0.25]
    hook.update_attribute("weight_1st_order", None)
    assert set(hook.objective({}, batch)) == {KEY_2ND}
    with pytest.raises(ValueError, match="not mutable"):
        hook.update_attribute("weight_3rd_order", 1.0)


def test_higher_rank_means_take_the_torch_expression(cusrl):
    """``[T, B, X, A]``: the reference's selection keeps the trailing dimensions; here two copies of a recorded case."""
    case = "T5,B3,A2|12|sequence"
    mean, done = case_inputs(case)
    stacked = torch.stack([mean, mean], dim=2)
    losses = make_hook(cusrl, *case_weights(case)).objective({}, {"curr_action_dist": {"mean": stacked}, "done": done})
    np.testing.assert_allclose(float(losses[KEY_1ST]), expected(case, "loss1"), rtol=1e-5)
    np.testing.assert_allclose(float(losses[KEY_2ND]), expected(case, "loss2"), rtol=1e-5)


def test_cpu_tensors_are_refused_outside_test_processes(cusrl, monkeypatch):
    monkeypatch.delenv("CUSRL_HOST_FORMS", raising=False)
    mean, done = case_inputs("T5,B3,A2|12|scalar")
    with pytest.raises(RuntimeError, match="ActionSmoothnessLoss received CPU tensors"):
        make_hook(cusrl, 0.1, None).objective({}, {"curr_action_dist": {"mean": mean}, "done": done})


def test_hook_name_and_place_in_a_factory(cusrl):
    """cusrl_test/hook/auxiliary/test_smoothness.py: two named instances, one registered after the other."""
    factory = cusrl.preset.RecurrentPpoAgentFactory().to_underlying()
    factory.register_hook(
        cusrl.hook.ActionSmoothnessLoss(weight_1st_order=0.01).name_("smoothness_loss_order1"), after="ppo_surrogate_loss",
    ).register_hook(
        cusrl.hook.ActionSmoothnessLoss(weight_2nd_order=[0.01] * 4).name_("smoothness_loss_order2"),
        after="smoothness_loss_order1",
    )
    assert factory.get_hook_index("smoothness_loss_order1") == factory.get_hook_index("ppo_surrogate_loss") + 1
    assert factory.get_hook_index("smoothness_loss_order1") == factory.get_hook_index("smoothness_loss_order2") - 1


def test_the_binding_exports_the_entry_and_its_sizing_helper(cusrl):
    from cusrl_amd import _native, ops

    assert {KERNEL, "cusrl_action_smoothness_workspace"} <= set(_native.EXPORTED_SYMBOLS)
    assert callable(ops.action_smoothness_fwd_bwd) and _native.ABI_VERSION == 7
    restype, argtypes = _native._PROTOTYPES[KERNEL]
    assert restype is _native.c_int and len(argtypes) == 12
    lib = _native.lib()
    # 8-byte words: {n_1, n_2} per count block (one per 256 envs, 64 at most) + two sums per walk block (one per 256 columns,
    # 1024 at most)
    assert lib.cusrl_action_smoothness_workspace(3, 1, 1) == 2 * (1 + 1)
    assert lib.cusrl_action_smoothness_workspace(8, 300, 7) == 2 * (2 + 9)
    assert lib.cusrl_action_smoothness_workspace(24, 16384, 12) == 2 * (64 + 768)
    assert lib.cusrl_action_smoothness_workspace(3, 1 << 20, 1) == 2 * (64 + 1024)
    assert lib.cusrl_action_smoothness_workspace(2, 4, 4) == 0  # fewer than 3 steps
    assert lib.cusrl_action_smoothness_workspace(3, 0, 4) == lib.cusrl_action_smoothness_workspace(3, 4, 0) == 0
    assert lib.cusrl_action_smoothness_workspace(1 << 12, 1 << 12, 1 << 8) == 0  # nothing beyond a 32-bit element index


def test_bad_arguments_are_refused_before_any_launch(cusrl):
    from cusrl_amd import _native

    lib = _native.lib()
    invalid, unsupported = _native._CONSTANTS["E_INVALID"], _native._CONSTANTS["E_UNSUPPORTED"]
    p = 0x1000  # a non-null placeholder: these calls return before touching it

    def call(**kw):
        pointers = {name: kw.get(name, p) for name in ("mean", "done", "w1", "w2", "losses", "counts", "d_mean", "workspace")}
        return lib.cusrl_action_smoothness_fwd_bwd(
            pointers["mean"], pointers["done"], pointers["w1"], pointers["w2"], kw.get("T", 4), kw.get("B", 2), kw.get("A", 3),
            pointers["losses"], pointers["counts"], pointers["d_mean"], pointers["workspace"], None)

    for name in ("mean", "done", "losses", "counts", "d_mean", "workspace"):
        assert call(**{name: None}) == invalid, name
    assert call(w1=None, w2=None) == invalid  # one weight may be absent, not both
    assert call(T=2) == invalid and call(T=0) == invalid and call(B=0) == invalid and call(A=-1) == invalid
    assert call(T=1 << 12, B=1 << 12, A=1 << 8) == unsupported
    assert invalid < 0 and unsupported < 0


def test_the_binding_refuses_host_tensors(cusrl):
    from cusrl_amd import ops

    mean, done = case_inputs("T5,B3,A2|12|scalar")
    with pytest.raises(RuntimeError, match="lives on cpu"):
        ops.action_smoothness_fwd_bwd(mean, done, torch.ones(2), None)
