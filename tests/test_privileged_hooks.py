"""The privileged-information hooks without a GPU: names, constructor / init errors in the reference's words, column-table
resolution, and every hook's host-form objective against the reference's recorded one (golden ``privileged.npz``)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _privileged import CASES, STATE, run_objective, stub_agent

NAMES = ("StateEstimation", "ReturnPrediction", "StatePrediction", "NextStatePrediction", "PolicyDistillationLoss")


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.mark.parametrize("name", NAMES)
def test_the_hooks_are_exported(cusrl, name):
    import cusrl_amd.hook.auxiliary as auxiliary

    assert getattr(cusrl, name) is getattr(cusrl.hook, name) is getattr(auxiliary, name)
    assert issubclass(getattr(cusrl, name), cusrl.Hook)
    assert name in cusrl.__all__ and name in cusrl.hook.__all__ and name in auxiliary.__all__


def test_the_binding_exports_the_kernel_and_its_sizing_helper(cusrl):
    from cusrl_amd import _native, ops

    assert {"cusrl_column_mse_fwd_bwd", "cusrl_column_mse_num_partials"} <= set(_native.EXPORTED_SYMBOLS)
    assert callable(ops.column_mse_fwd_bwd) and _native.ABI_VERSION == 7
    lib = _native.lib()
    # the launch rule of cusrl_mse_loss_num_partials on rows * K elements; nothing beyond a 32-bit element index
    assert lib.cusrl_column_mse_num_partials(37, 5) == 1 and lib.cusrl_column_mse_num_partials(1820, 9) == 1
    assert lib.cusrl_column_mse_num_partials(2049, 9) == lib.cusrl_mse_loss_num_partials(2049 * 9) == 10
    assert lib.cusrl_column_mse_num_partials(70000, 31) == 1024
    assert lib.cusrl_column_mse_num_partials(0, 4) == lib.cusrl_column_mse_num_partials(4, 0) == 0
    assert lib.cusrl_column_mse_num_partials(1 << 30, 4) == 0
    # argument errors are refused before anything is launched: INVALID (-1) / UNSUPPORTED
    invalid, unsupported = _native._CONSTANTS["E_INVALID"], _native._CONSTANTS["E_UNSUPPORTED"]
    assert lib.cusrl_column_mse_fwd_bwd(None, None, 4, None, 2, 4, 1.0, None, None, None, None) == invalid
    assert lib.cusrl_column_mse_fwd_bwd(8, 8, 4, None, 0, 4, 1.0, 8, 8, 8, None) == invalid
    assert lib.cusrl_column_mse_fwd_bwd(8, 8, 3, None, 2, 4, 1.0, 8, 8, 8, None) == invalid  # pitch < K without a table
    assert lib.cusrl_column_mse_fwd_bwd(8, 8, 4, None, 1 << 30, 4, 1.0, 8, 8, 8, None) == unsupported


@pytest.mark.parametrize("indices", [slice(None), slice(2, 9, 3), [5, 0, 5], slice(None, None, -1), torch.tensor([3, -1])],
                         ids=["all", "strided", "list", "reversed", "tensor"])
def test_column_resolution(cusrl, indices):
    from cusrl_amd import ops
    from cusrl_amd.hook.auxiliary._column_mse import ColumnSelection

    C = 11
    selection = ColumnSelection(indices, C)
    if isinstance(indices, slice) and indices == slice(None):
        assert selection.columns is None and selection.dim == C and selection.table("cpu") is None
        return
    if isinstance(indices, slice) and (indices.step or 1) < 0:
        expected = torch.arange(C).flip(0)  # torch's own indexing refuses a negative step; what the slice means in Python
        assert list(range(C))[indices] == expected.tolist()
    else:
        expected = torch.arange(C)[indices]
    assert selection.columns.dtype == torch.int32 and selection.columns.tolist() == expected.tolist()
    assert selection.dim == expected.numel()
    x = torch.randn(4, C)
    assert torch.equal(x[..., selection.torch_index()], x[..., expected])
    assert ops.resolve_columns(indices, C).tolist() == expected.tolist()
    with pytest.raises(ValueError, match="selects no column"):
        ColumnSelection(slice(3, 3), C)


def test_constructor_and_init_errors_are_the_references(cusrl):
    agent = stub_agent(cusrl)
    hook = cusrl.StateEstimation(cusrl.Mlp.Factory([8]), source_name="proprioception")
    hook.pre_init(agent)
    with pytest.raises(ValueError, match=r"^'source_dim' must be specified for source_name 'proprioception'\.$"):
        hook.init()
    hook = cusrl.StateEstimation(cusrl.Mlp.Factory([8]), target_name="contact")
    hook.pre_init(agent)
    with pytest.raises(ValueError, match=r"^'target_dim' must be specified for target_name 'contact'\.$"):
        hook.init()
    agent.has_state = False
    for hook, message in ((cusrl.StatePrediction([0]), "StatePrediction requires the state space defined"),
                          (cusrl.NextStatePrediction([0]), "NextStatePrediction requires the agent to define a state space")):
        hook.pre_init(agent)
        with pytest.raises(ValueError, match=f"^{message}$"):
            hook.init()
    with pytest.raises(TypeError):
        cusrl.StatePrediction()  # target_indices has no default
    for name in NAMES:  # `weight` is the one mutable attribute of all five
        hook = getattr(cusrl, name)(*([cusrl.Mlp.Factory([8])] if name == "StateEstimation" else [[0]] if "State" in name else []))
        hook.update_attribute("weight", 0.125)
        assert hook.weight == 0.125 and hook._mutable == {"weight"}
    defaults = {"StateEstimation": 1.0, "ReturnPrediction": 0.01, "StatePrediction": 0.01, "NextStatePrediction": 0.01,
                "PolicyDistillationLoss": 1.0}
    assert cusrl.PolicyDistillationLoss().target_name == "expert_action"
    assert cusrl.ReturnPrediction().latent_name == "backbone.output" and not cusrl.ReturnPrediction().predicts_value_instead_of_return
    for name, weight in defaults.items():
        hook = getattr(cusrl, name)(*([cusrl.Mlp.Factory([8])] if name == "StateEstimation" else [[0]] if "State" in name else []))
        assert hook.weight == weight


def test_state_estimation_dims_keys_and_the_refused_recurrent_estimator(cusrl):
    agent = stub_agent(cusrl)
    hook = cusrl.StateEstimation(cusrl.Mlp.Factory([8]), source_name="next_state", source_indices=[0, 3], target_name="observation",
                                 target_indices=slice(4, 10), estimation_name="guess")
    hook.pre_init(agent)
    hook.init()
    assert (hook.source_dim, hook.target_dim) == (STATE, 16)
    assert (hook.estimator.input_dim, hook.estimator.output_dim) == (2, 6)
    assert [name for name, _ in hook.named_parameters()][0].startswith("estimator.")
    transition = {"next_state": torch.randn(5, STATE)}
    hook.pre_act(transition)
    # a feed-forward estimator has no memory: the key is there and None, so the buffer stores no `*_memory` leaf
    assert transition["guess"].shape == (5, 6) and "estimator_memory" in transition and transition["estimator_memory"] is None
    hook.post_step({"done": torch.zeros(5, 1, dtype=torch.bool)})
    assert hook.post_step_device_free
    recurrent = cusrl.StateEstimation(cusrl.nn.Rnn.Factory("GRU", num_layers=1, hidden_size=8))
    recurrent.pre_init(agent)
    with pytest.raises(NotImplementedError, match="StateEstimation does not support recurrent estimators yet"):
        recurrent.init()


def test_the_latent_probe_finds_the_latent_and_leaves_the_actor_as_it_was(cusrl):
    agent = stub_agent(cusrl)
    assert agent.actor.fused_inference
    for hook, width in ((cusrl.ReturnPrediction(), 1), (cusrl.StatePrediction([5, 0, 5]), 3), (cusrl.NextStatePrediction(slice(2, 5)), 3)):
        hook.pre_init(agent)
        hook.init()
        inner = hook.predictor.wrapped if isinstance(hook, cusrl.NextStatePrediction) else hook.predictor
        assert type(inner) is torch.nn.Linear  # the reference's default factory
        assert (inner.in_features, inner.out_features) == (16 + 8 * isinstance(hook, cusrl.NextStatePrediction), width)
    assert agent.actor.fused_inference and not agent.actor.intermediate_repr


@pytest.mark.parametrize("hook_kind,form", CASES, ids=[f"{kind}-{form}" for kind, form in CASES])
def test_host_form_objective_reproduces_the_reference(cusrl, golden, hook_kind, form):
    torch.manual_seed(0)
    loss, grads, expected = run_objective(cusrl, golden("privileged"), hook_kind, form)
    np.testing.assert_allclose(loss.item(), expected, rtol=1e-6)
    for name, (got, reference) in grads.items():
        # the same torch expression on the same inputs: the reference's gradient as torch computes it
        np.testing.assert_allclose(got.numpy(), reference, rtol=1e-6, atol=1e-9, err_msg=f"{hook_kind} {form} {name}")
    if hook_kind == "distillation":
        assert np.array_equal(grads["d_mean"][0].numpy(), grads["d_mean"][1])


def test_temporal_batches_and_a_user_criterion_keep_the_torch_expression(cusrl):
    agent = stub_agent(cusrl)
    hook = cusrl.NextStatePrediction(slice(None, None, -1), weight=0.5)
    hook.pre_init(agent)
    hook.init()
    latent, action, next_state = torch.randn(3, 7, 16), torch.randn(3, 7, 8), torch.randn(3, 7, STATE)
    agent.actor.intermediate_repr["backbone.output"] = latent
    loss = hook.objective({"temporal": True}, {"next_state": next_state, "action": action})["next_state_prediction_loss"]
    expected = torch.nn.functional.mse_loss(hook.predictor(latent, action), next_state.flip(-1)) * 0.5
    assert torch.equal(loss, expected)
    hook.criterion = torch.nn.SmoothL1Loss()
    loss = hook.objective({}, {"next_state": next_state, "action": action})["next_state_prediction_loss"]
    assert torch.equal(loss, torch.nn.functional.smooth_l1_loss(hook.predictor(latent, action), next_state.flip(-1)) * 0.5)
