"""``ActionSmoothnessLoss`` on the device against the reference's recorded losses, counts and autograd gradients (golden
``smoothness.npz``): every case through the public hook in one ``cusrl_action_smoothness_fwd_bwd`` call, the binding's counts
and per-term gradient planes, reproducibility, a strided mean, a rescaled loss, weights changed under a captured launch, and
a short recurrent training run.  Bounds: 1e-5 relative for a loss, 1e-5 of the largest entry for a gradient — the project's
standing ones; counts are exact; an empty selection is NaN with an all-zero gradient, as recorded."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _smoothness import (CASES, INPUTS, KEY_1ST, KEY_2ND, case_inputs, case_weights, check_case, expected, make_hook, parse,
                         run_case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = "cusrl_action_smoothness_fwd_bwd"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name=KERNEL):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _device_weights(case, action_dim):
    """The two ``[A]`` fp32 device vectors of a case's weights (None where the case gives none)."""
    return tuple(None if w is None else torch.as_tensor(w, dtype=torch.float32).expand(action_dim).contiguous().to(DEV)
                 for w in case_weights(case))


@pytest.mark.parametrize("case", CASES)
def test_the_hook_on_the_device_reproduces_the_reference(cusrl, case, gradient_parity):
    before = _count()
    losses, d_mean = run_case(cusrl, case, device=DEV)
    assert _count() == before + 1  # the HIP form: one call for both terms and their gradients
    assert all(loss.shape == () and loss.is_cuda for loss in losses.values())
    check_case(case, losses, d_mean, None, gradient_parity, case)


@pytest.mark.parametrize("name", INPUTS)
def test_the_binding_counts_exactly_and_repeats_bit_for_bit(cusrl, name, gradient_parity):
    """Both terms through ``ops``: the counts, one gradient plane per term whose sum is the recorded gradient, the planes of the
    single-term calls bit for bit, and two calls on the same inputs bit-identical."""
    from cusrl_amd import ops

    case = f"{name}|12|sequence"
    mean, done = case_inputs(case, DEV)
    w1, w2 = _device_weights(case, mean.shape[-1])
    losses, counts, d_mean = ops.action_smoothness_fwd_bwd(mean, done, w1, w2)
    assert losses.shape == (2,) and counts.dtype == torch.int64 and d_mean.shape == (2, *mean.shape)
    check_case(case, {KEY_1ST: losses[0], KEY_2ND: losses[1]}, d_mean[0] + d_mean[1], counts.tolist(), gradient_parity,
               f"ops,{case}")
    again = ops.action_smoothness_fwd_bwd(mean, done, w1, w2)
    assert torch.equal(losses.view(torch.int32), again[0].view(torch.int32)), "two calls on the same inputs differ"  # (NaN too)
    assert torch.equal(counts, again[1]) and torch.equal(d_mean, again[2])
    only1 = ops.action_smoothness_fwd_bwd(mean, done, w1, None)
    only2 = ops.action_smoothness_fwd_bwd(mean, done, None, w2)
    assert only1[2].shape == only2[2].shape == (1, *mean.shape)
    assert torch.equal(only1[2][0], d_mean[0]) and torch.equal(only2[2][0], d_mean[1])
    assert torch.equal(only1[0][:1].view(torch.int32), losses[:1].view(torch.int32)) and only1[0][1] == 0
    assert torch.equal(only2[0][1:].view(torch.int32), losses[1:].view(torch.int32)) and only2[0][0] == 0
    assert torch.equal(only1[1], counts) and torch.equal(only2[1], counts)


def test_a_column_slice_of_a_wider_tensor_gives_the_same_values(cusrl):
    from cusrl_amd import ops

    case = "T24,B37,A12|12|sequence"
    mean, done = case_inputs(case, DEV)
    wide = torch.randn(*mean.shape[:2], mean.shape[2] + 5, device=DEV)
    wide[..., 3:3 + mean.shape[2]] = mean
    view = wide[..., 3:3 + mean.shape[2]]
    assert not view.is_contiguous() and torch.equal(view, mean)
    w1, w2 = _device_weights(case, mean.shape[-1])
    strided, contiguous = (ops.action_smoothness_fwd_bwd(m, done, w1, w2) for m in (view, mean))
    assert all(torch.equal(a, b) for a, b in zip(strided, contiguous))
    # and through the hook, whose gradient arrives in the wide leaf
    hook = make_hook(cusrl, *case_weights(case), device=DEV, action_dim=mean.shape[-1])
    wide.requires_grad_()
    losses = hook.objective({}, {"curr_action_dist": {"mean": wide[..., 3:3 + mean.shape[2]]}, "done": done})
    sum(losses.values()).backward()
    assert torch.equal(wide.grad[..., 3:3 + mean.shape[2]], contiguous[2][0] + contiguous[2][1])
    assert not wide.grad[..., :3].any() and not wide.grad[..., 3 + mean.shape[2]:].any()


@pytest.mark.parametrize("case", ["T8,B300,A7|12|scalar", "T5,B3,A2|2|sequence"])
def test_a_rescaled_loss_scales_the_gradient(cusrl, case, gradient_parity):
    losses, d_mean = run_case(cusrl, case, device=DEV, scale=3.0)
    check_case(case, losses, d_mean, None, gradient_parity, f"{case},x3", scale=3.0)


def test_each_term_is_scaled_by_its_own_incoming_gradient(cusrl, gradient_parity):
    case = "T24,B37,A12|12|sequence"
    mean, done = case_inputs(case, DEV)
    hook = make_hook(cusrl, *case_weights(case), device=DEV, action_dim=mean.shape[-1])
    mean.requires_grad_()
    losses = hook.objective({}, {"curr_action_dist": {"mean": mean}, "done": done})
    (2.0 * losses[KEY_1ST] - 0.5 * losses[KEY_2ND]).backward()
    reference = 2.0 * expected("T24,B37,A12|1|sequence", "d_mean") - 0.5 * expected("T24,B37,A12|2|sequence", "d_mean")
    gradient_parity("smoothness.d_mean[per-term scales]", mean.grad.cpu().numpy(), reference, 1e-5)


def test_other_forms_keep_the_torch_expression(cusrl, gradient_parity):
    case = "T5,B3,A2|12|sequence"
    mean, done = case_inputs(case, DEV)
    hook = make_hook(cusrl, *case_weights(case), device=DEV, action_dim=mean.shape[-1])
    before = _count()
    losses = hook.objective({}, {"curr_action_dist": {"mean": mean.double()}, "done": done})
    assert _count() == before and losses[KEY_1ST].dtype == torch.float64
    np.testing.assert_allclose(losses[KEY_1ST].item(), expected(case, "loss1"), rtol=1e-5)
    np.testing.assert_allclose(losses[KEY_2ND].item(), expected(case, "loss2"), rtol=1e-5)
    stacked = torch.stack([mean, mean], dim=2)
    losses = hook.objective({}, {"curr_action_dist": {"mean": stacked}, "done": done})
    assert _count() == before
    np.testing.assert_allclose(losses[KEY_2ND].item(), expected(case, "loss2"), rtol=1e-5)
    with pytest.raises(RuntimeError, match="received CPU tensors"):  # the gate is shut in a GPU test, as in a user's process
        hook.objective({}, {"curr_action_dist": {"mean": mean.cpu()}, "done": done.cpu()})


def test_update_attribute_rewrites_the_device_weights_in_place(cusrl):
    case = "T5,B3,A2|12|scalar"
    mean, done = case_inputs(case, DEV)
    batch = {"curr_action_dist": {"mean": mean}, "done": done}
    hook = make_hook(cusrl, *case_weights(case), device=DEV, action_dim=mean.shape[-1])
    vectors = dict(hook._device_weights)
    assert len(vectors) == 2 and all(v.is_cuda and v.shape == (2,) for v in vectors.values())  # uploaded at init
    first = hook.objective({}, batch)
    hook.update_attribute("weight_2nd_order", [0.5, 0.25])
    assert {k: v.data_ptr() for k, v in hook._device_weights.items()} == {k: v.data_ptr() for k, v in vectors.items()}
    second = hook.objective({}, batch)
    assert torch.equal(second[KEY_1ST], first[KEY_1ST]) and not torch.equal(second[KEY_2ND], first[KEY_2ND])
    from _smoothness import closed_form_f64

    reference = closed_form_f64(mean.cpu().numpy(), done.cpu().numpy(), None, [0.5, 0.25])["loss2"]
    np.testing.assert_allclose(second[KEY_2ND].item(), reference, rtol=1e-5)


@pytest.mark.parametrize("name", ["T8,B300,A7", "T5,B3,A2"])
def test_a_captured_replay_equals_eager_and_reads_changed_weights(cusrl, name):
    """The ``ops`` call on one stream in a graph (count, walk and — beyond one block — finalize: kernel nodes only), replayed;
    then the weight vectors are rewritten in place, outside any capture, and the same graph gives the new weights' result."""
    from cusrl_amd import ops

    case, other = f"{name}|12|sequence", f"{name}|12|scalar"
    mean, done = case_inputs(case, DEV)
    w1, w2 = _device_weights(case, mean.shape[-1])
    new_w1, new_w2 = _device_weights(other, mean.shape[-1])
    eager = ops.action_smoothness_fwd_bwd(mean, done, w1, w2)
    eager_new = ops.action_smoothness_fwd_bwd(mean, done, new_w1, new_w2)
    assert not torch.equal(eager[2], eager_new[2])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.action_smoothness_fwd_bwd(mean, done, w1, w2)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=stream):
        losses, counts, d_mean = ops.action_smoothness_fwd_bwd(mean, done, w1, w2)
    census = ops.graph_census(graph)
    assert census["memset"] == 0 and census["kernel"] == (3 if name == "T8,B300,A7" else 2), census
    graph.instantiate()
    for expected_result in (eager, eager_new):
        losses.fill_(float("nan"))
        counts.zero_()
        d_mean.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((losses, counts, d_mean), expected_result))
        w1.copy_(new_w1)
        w2.copy_(new_w2)


def test_a_recurrent_agent_trains_with_the_hook(cusrl):
    """GRU, hidden size 32, 8 envs, T = 8, the dummy env, two iterations: both terms reach the update's metrics, and the entry
    is called once per minibatch step."""
    cusrl.set_global_seed(3)
    iterations, epochs, mini_batches = 2, 2, 2
    factory = cusrl.preset.RecurrentPpoAgentFactory(
        rnn_type="GRU", actor_hidden_size=32, critic_hidden_size=32, num_steps_per_update=8, sampler_epochs=epochs,
        sampler_mini_batches=mini_batches).to_underlying()
    factory.register_hook(cusrl.hook.ActionSmoothnessLoss(weight_1st_order=0.01, weight_2nd_order=[0.01] * 4),
                          after="on_policy_preparation")
    assert factory.get_hook_index("action_smoothness_loss") == factory.get_hook_index("on_policy_preparation") + 1
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=10, action_dim=4, device=DEV)
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    before = _count()
    trainer.run_training_loop()
    assert _count() == before + iterations * epochs * mini_batches
    for key in (KEY_1ST, KEY_2ND):
        assert np.isfinite(trainer.last_info[f"Agent/{key}"]), (key, trainer.last_info)
    assert np.isfinite(trainer.last_info["Agent/value_loss"])
