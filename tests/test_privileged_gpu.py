"""The privileged-information hooks on the device: ``cusrl_column_mse_fwd_bwd`` against a float64 evaluation of its formula on
the host, every hook's recorded stand-alone objective, replays of the reference's update traces (golden ``privileged.npz``:
(pa) StateEstimation, (pb) StatePrediction + ReturnPrediction, (pc) NextStatePrediction + PolicyDistillationLoss) and short
training runs under ``compile=True``.  Bounds: 1e-5 relative for a loss, 1e-5 of the largest entry for a gradient — the
project's standing ones; the trace replays hold what tests/test_symmetry_trace_gpu.py holds for the same quantities."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _privileged import AUX_KEYS, CASES, STATE, column_mse_f64, privileged_hooks, run_objective
from test_agent_gpu import build_agent_from_golden, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = "cusrl_column_mse_fwd_bwd"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name=KERNEL):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _case(name):
    """``(prediction, target, column list | None)`` on the device; every shape is there for a path that can go wrong."""
    gen = torch.Generator().manual_seed(17)

    def randn(*shape):
        return (torch.randn(*shape, generator=gen) * 1.3 + 0.2).to(DEV)

    if name == "one_block_ragged_repeated":  # one self-finalising block, a ragged tail, a repeated column
        return randn(37, 5), randn(37, 11), [5, 0, 5, 10, 3]
    if name == "smallest":
        return randn(1, 1), randn(1, 1), None
    if name == "first_multi_block":  # 18441 elements: 10 blocks, the last one ragged, then the finalize launch
        return randn(2049, 9), randn(2049, 16), None
    if name == "vector":  # no table, K % 4 == 0, pitch % 4 == 0, aligned pointers
        prediction, target = randn(512, 8), randn(512, 8)
        assert prediction.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 0
        return prediction, target, None
    if name == "unaligned":  # the same shape from a target view offset by one float
        target = randn(512 * 8 + 1)[1:].view(512, 8)
        assert target.data_ptr() % 16 == 4
        return randn(512, 8), target, None
    if name == "leaf_view":  # columns 2..9 of a 16-wide leaf, read in place through the pitch
        leaf = randn(300, 16)
        return randn(300, 8), leaf[:, 2:10], None
    if name == "grid_stride":  # 2.17 M elements: past the 1024-block cap, 8.3 elements per thread
        return randn(70000, 31), randn(70000, 40), torch.randperm(40, generator=gen)[:31].tolist()
    if name == "temporal":  # a [T, B, K] prediction of a recurrent actor: rows = T * B
        return randn(3, 7, 5), randn(3, 7, 11), [10, 2, 2, 0, 7]
    raise KeyError(name)


KERNEL_CASES = ["one_block_ragged_repeated", "smallest", "first_multi_block", "vector", "unaligned", "leaf_view", "grid_stride",
                "temporal"]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_column_mse_matches_float64(cusrl, name, gradient_parity):
    from cusrl_amd import ops

    prediction, target, column_list = _case(name)
    columns = None if column_list is None else ops.column_table(column_list, target.shape[-1], DEV)
    weight = 0.37
    before = _count()
    loss, grad = ops.column_mse_fwd_bwd(prediction, target, columns, weight)
    assert _count() == before + 1
    if name == "leaf_view":
        assert not target.is_contiguous()  # (nothing was staged: the view itself was read)
    again = ops.column_mse_fwd_bwd(prediction, target, columns, weight)
    assert torch.equal(loss, again[0]) and torch.equal(grad, again[1]), "two calls on the same inputs differ"
    ref_loss, ref_grad = column_mse_f64(prediction, target, column_list, weight)
    assert grad.shape == prediction.shape and loss.shape == ()
    print(f"{name}: loss {loss.item():.9g} vs {ref_loss:.9g} (rel {abs(loss.item() - ref_loss) / abs(ref_loss):.2e})")
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-5)
    gradient_parity(f"column_mse.d_prediction[{name}]", host(grad), ref_grad, 1e-5)


@pytest.mark.parametrize("name", ["one_block_ragged_repeated", "first_multi_block", "vector"])
def test_column_mse_replays_bit_identically_from_a_graph(cusrl, name):
    from cusrl_amd import ops

    prediction, target, column_list = _case(name)
    columns = None if column_list is None else ops.column_table(column_list, target.shape[-1], DEV)
    eager_loss, eager_grad = ops.column_mse_fwd_bwd(prediction, target, columns, 0.8)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.column_mse_fwd_bwd(prediction, target, columns, 0.8)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=stream):
        loss, grad = ops.column_mse_fwd_bwd(prediction, target, columns, 0.8)
    census = ops.graph_census(graph)
    assert census["memset"] == 0, census  # partials and finalize: nothing to zero
    graph.instantiate()
    for _ in range(3):
        loss.fill_(float("nan"))
        grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager_loss) and torch.equal(grad, eager_grad)


def test_column_mse_refuses_what_it_cannot_take(cusrl):
    from cusrl_amd import ops

    prediction, target = torch.randn(6, 3, device=DEV), torch.randn(6, 5, device=DEV)
    before = _count()
    with pytest.raises(IndexError, match="out of range"):
        ops.column_mse_fwd_bwd(prediction, target, torch.tensor([0, 5, 1], dtype=torch.int32, device=DEV), 1.0)
    with pytest.raises(ValueError, match="columns for a"):
        ops.column_mse_fwd_bwd(prediction, target, ops.column_table([0, 1], 5, DEV), 1.0)
    with pytest.raises(ValueError, match="leading shape"):
        ops.column_mse_fwd_bwd(prediction, target[:5], None, 1.0)
    with pytest.raises(ValueError, match="wide target"):
        ops.column_mse_fwd_bwd(target, prediction, None, 1.0)
    with pytest.raises(TypeError):
        ops.column_mse_fwd_bwd(prediction, target, torch.tensor([0, 1, 2], device=DEV), 1.0)  # int64 table
    with pytest.raises(RuntimeError, match="lives on cpu"):
        ops.column_mse_fwd_bwd(prediction.cpu(), target, None, 1.0)
    assert _count() == before  # nothing reached the device


@pytest.mark.parametrize("hook_kind,form", CASES, ids=[f"{kind}-{form}" for kind, form in CASES])
def test_hook_objective_on_the_device_reproduces_the_reference(cusrl, golden, hook_kind, form, gradient_parity):
    before = _count()
    loss, grads, expected = run_objective(cusrl, golden("privileged"), hook_kind, form, device=DEV)
    assert _count() == before + 1  # the HIP form, one launch for loss and gradient
    np.testing.assert_allclose(loss.item(), expected, rtol=1e-5)
    for name, (got, reference) in grads.items():
        gradient_parity(f"privileged.objective.{name}[{hook_kind},{form}]", host(got), reference, 1e-5)


def test_a_rescaled_loss_and_a_user_criterion(cusrl, golden, gradient_parity):
    """Anything but the agent's unit gradient is multiplied in; a criterion of the user's keeps torch's expression."""
    hook = cusrl.hook.PolicyDistillationLoss(weight=1.5)
    hook.init()
    g = golden("privileged")
    mean = torch.from_numpy(g["obj_distillation_mean"]).to(DEV).requires_grad_()
    batch = {"curr_action_dist": {"mean": mean}, "expert_action": torch.from_numpy(g["obj_expert_action"]).to(DEV)}
    (hook.objective({}, batch)["distillation_loss"] * 3.0).backward()
    gradient_parity("privileged.rescaled.d_mean", host(mean.grad), 3.0 * g["obj_distillation_d_mean"], 1e-5)
    hook.criterion = torch.nn.MSELoss(reduction="sum")
    before = _count()
    loss = hook.objective({}, batch)["distillation_loss"]
    assert _count() == before
    np.testing.assert_allclose(loss.item(), g["obj_distillation_loss"] * mean.numel(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------ update traces
MODES = ["fused", "hook_by_hook", "hipgraph", "flat_adam"]


class _WithState:
    """The package as ``build_agent_from_golden`` sees it, but its environment spec carries the trace's privileged state."""

    def __init__(self, module):
        self._module = module

        def spec(observation_dim, action_dim, **kwargs):
            return module.EnvironmentSpec(observation_dim, action_dim, state_dim=STATE, **kwargs)

        self.EnvironmentSpec = spec

    def __getattr__(self, name):
        return getattr(self._module, name)


@pytest.mark.parametrize("tag", list(AUX_KEYS))
@pytest.mark.parametrize("mode", MODES)
def test_privileged_update_replays_reference_trace(cusrl, golden, tag, mode, gradient_parity):
    from cusrl_amd.hook.on_policy.fused import FusedPpoObjective

    g = golden("privileged")
    overrides = {"compile": True} if mode == "hipgraph" else {"optimizer_kwargs": {"fused": True}} if mode == "flat_adam" else {}
    agent, trace = build_agent_from_golden(_WithState(cusrl), g, tag, extra_hooks=privileged_hooks(cusrl, tag), **overrides)
    assert agent.has_state and "estimator_memory" not in agent.buffer.storage
    agent.fuse_objective = mode != "hook_by_hook"
    if mode != "hook_by_hook":
        assert FusedPpoObjective.mode(agent.hook) == "split"  # the stock terms stay one fused launch beside the new hooks

    keys = AUX_KEYS[tag]
    per_step, aux_losses = [], []
    inner = agent.hook.objective

    def counted(metadata, batch):
        before = _count(), _count("cusrl_ppo_loss_fwd_bwd")
        result = inner(metadata, batch)
        per_step.append((_count() - before[0], _count("cusrl_ppo_loss_fwd_bwd") - before[1]))
        if result["value_loss"] is not None:
            aux_losses.append(torch.stack([result[key] for key in keys]).detach().clone())
        return result

    agent.hook.objective = counted
    torch.manual_seed(99)
    metrics = agent.update()

    assert np.array_equal(host(torch.stack(trace["indices"])), g[tag + "_indices"]), "minibatch permutations differ"
    # exactly one launch per hook and minibatch step; the stock terms one fused launch (none when evaluated hook by hook)
    assert per_step and all(launched == len(keys) for launched, _ in per_step), per_step
    assert all(fused == (mode != "hook_by_hook") for _, fused in per_step), per_step
    seen = len(trace["objectives"])
    assert seen == (len(g[tag + "_objectives"]) if not agent._graphed_steps else sum(1 for s in agent._graphed_steps.values()))
    np.testing.assert_allclose(host(torch.stack(trace["objectives"])), g[tag + "_objectives"][:seen], rtol=2e-5, atol=1e-6)
    assert len(aux_losses) == seen
    np.testing.assert_allclose(host(torch.stack(aux_losses)), g[tag + "_aux"][:seen], rtol=2e-5, atol=1e-6)
    clipped = g[tag + ("_grads_unclipped" if agent.flat_optimizer is not None else "_grads")]
    assert len(trace["grads_unclipped"]) == len(g[tag + "_grads_unclipped"])
    for step, (raw, after) in enumerate(zip(trace["grads_unclipped"], trace["grads"])):
        gradient_parity(f"privileged.grads_unclipped[{tag},{mode},{step}]", host(raw), g[tag + "_grads_unclipped"][step], 1e-5)
        gradient_parity(f"privileged.grads[{tag},{mode},{step}]", host(after), clipped[step], 1e-5)
    np.testing.assert_allclose(host(torch.stack(trace["params_after"])), g[tag + "_params_after"], rtol=1e-4, atol=2e-6)
    ref = dict(zip((str(k) for k in g[tag + "_metric_keys"]), g[tag + "_metric_vals"]))
    for key in ("value_loss", "surrogate_loss", "entropy_loss", *keys):
        np.testing.assert_allclose(metrics["Agent/" + key], ref["Agent/" + key], rtol=1e-3, atol=1e-5, err_msg=key)


# ------------------------------------------------------------------------------------------------ training under compile=True
def _train(cusrl, tag, iterations):
    cusrl.set_global_seed(7)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=64, observation_dim=16, action_dim=8, state_dim=STATE, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2, compile=True,
                                           optimizer_kwargs={"capturable": True, "fused": True}).to_underlying()
    for hook, where in privileged_hooks(cusrl, tag):
        factory.register_hook(hook, **where)
    before = _count()
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    trainer.run_training_loop()
    assert _count() > before
    info = trainer.last_info
    for key in AUX_KEYS[tag] + ("value_loss", "surrogate_loss"):
        assert any(k.endswith(key) for k in info), key
    for key, value in info.items():
        if "loss" in key:
            assert np.isfinite(value), key
    for _, p in trainer.agent.named_parameters():
        assert torch.isfinite(p).all()
    return trainer


@pytest.mark.parametrize("tag", ["pb", "pc"])
def test_training_with_representation_hooks_under_compile(cusrl, tag):
    trainer = _train(cusrl, tag, iterations=2)
    assert trainer.agent._graphed_steps  # the minibatch steps were captured with the hooks inside


def test_state_estimation_trains_and_keeps_the_captured_rollout(cusrl):
    # (4 iterations: a step's graph exists from its third use, the whole-rollout graph is built on top of all of them)
    trainer = _train(cusrl, "pa", iterations=4)
    agent = trainer.agent
    assert "state_estimation" in agent.buffer.storage and "estimator_memory" not in agent.buffer.storage
    graphed = trainer._graphed_rollout
    assert graphed is not None and graphed.captured > 0 and len(graphed.rollouts) == 1  # the whole rollout, one graph
    estimator_params = [p for name, p in agent.named_parameters() if "state_estimation.estimator" in name]
    assert estimator_params and agent.flat_gradients is not None
    flat_ids = {id(p) for p in agent.flat_gradients.params}
    assert all(id(p) in flat_ids for p in estimator_params)  # their window of the flat gradient buffer, like RND's predictor


def test_a_changed_weight_sends_the_captured_regions_back_to_capture(cusrl):
    """``weight`` is a registered mutable of all five hooks: a schedule's ``update_attribute`` changes the signature every
    captured region is replayed under (graphs.capture_signature), so the next update captures the new value."""
    from cusrl_amd.template.graphs import capture_signature

    spec = cusrl.EnvironmentSpec(16, 8, state_dim=STATE, num_instances=8, device=DEV)
    for tag in AUX_KEYS:
        factory = cusrl.preset.PpoAgentFactory(device=DEV).to_underlying()
        for hook, where in privileged_hooks(cusrl, tag):
            factory.register_hook(hook, **where)
        agent = factory(spec)
        for hook in agent.hook:
            if "weight" in hook._mutable and type(hook).__module__.startswith("cusrl_amd.hook.auxiliary"):
                before = capture_signature(agent)
                hook.update_attribute("weight", hook.weight * 0.5)
                assert capture_signature(agent) != before, hook.name
