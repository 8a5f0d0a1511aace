"""The control hooks and their schedulers without a GPU: scheduler values against the reference's recorded ones (golden
``control_hooks.npz``), constructor validation, naming, and the host logic of every hook driven by hand on CPU agents and fake
hooks (the hot path refuses CPU tensors, so nothing here runs an update)."""

from __future__ import annotations

import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _control_hooks as shared
import cusrl_amd as cusrl
from cusrl_amd.template.hook import Hook, HookComposite
from cusrl_amd.utils import scheduler as schedulers

SPEC = dict(num_instances=shared.ENVS, device="cpu")


def _agent(config=None, extra=()):
    return shared.factory(cusrl, config, "cpu", extra)(cusrl.EnvironmentSpec(shared.OBS, shared.ACT, **SPEC))


# ------------------------------------------------------------------------------------------------ schedulers
@pytest.mark.parametrize("name", list(shared.scheduler_cases(schedulers)))
def test_scheduler_values_equal_the_reference_exactly(golden, name):
    g = golden("control_hooks")
    assert list(g["scheduler_names"]) == list(shared.scheduler_cases(schedulers))
    scheduler = shared.scheduler_cases(schedulers)[name]
    iterations = [int(i) for i in g["scheduler_iterations"]]
    assert iterations == list(range(-1, 13))
    values, expected = [scheduler(i) for i in iterations], g["scheduler/" + name]
    if expected.dtype == bool:
        assert all(isinstance(v, bool) for v in values) and values == expected.tolist()
    else:  # the same Python float expressions in the same order: the same bits
        assert np.array_equal(np.array(values, dtype=np.float64).view(np.uint64), expected.view(np.uint64)), (values, expected)


def test_schedulers_hit_their_anchors_and_hold_outside():
    cases = shared.scheduler_cases(schedulers)
    assert [cases["step"](i) for i in (-1, 1, 2, 8, 9, 12)] == [0.01, 0.01, 0.5, 0.5, 0.0, 0.0]
    assert [cases["piecewise"](i) for i in (-1, 2, 5, 9, 12)] == [0.01, 0.01, 0.3, 0.0, 0.0]
    for name, (first, last) in {"cosine": (0.01, 0.7), "tanh_half": (0.01, 0.7), "tanh_three": (0.7, 0.01)}.items():
        assert cases[name](-1) == cases[name](2) == first and cases[name](9) == cases[name](12) == last
        inside = [cases[name](i) for i in range(3, 9)]
        assert all(min(first, last) < v < max(first, last) for v in inside)
        assert inside == sorted(inside, reverse=first > last)
    assert schedulers.StepScheduler("a", (3, "b"))(3) == "b"  # (any value type)
    assert cusrl.utils.StepScheduler is schedulers.StepScheduler and cusrl.utils.scheduler is schedulers


@pytest.mark.parametrize("build, message", [
    (lambda: schedulers.StepScheduler(0.0, (3, 1.0), (3, 2.0)), "step coordinates must be strictly increasing"),
    (lambda: schedulers.StepScheduler(0.0, (4, 1.0), (3, 2.0)), "step coordinates must be strictly increasing"),
    (lambda: schedulers.PiecewiseLinearScheduler((2, 0.0), (2, 1.0)), "step coordinates must be strictly increasing"),
    (lambda: schedulers.PiecewiseLinearScheduler((0, 0.0), (5, 1.0), (4, 1.0)), "step coordinates must be strictly increasing"),
    (lambda: schedulers.CosineAnnealingScheduler((5, 0.0), (5, 1.0)), "step coordinates must be strictly increasing"),
    (lambda: schedulers.TanhScheduler((6, 0.0), (5, 1.0), 1.0), "step coordinates must be strictly increasing"),
    (lambda: schedulers.PiecewiseLinearScheduler((0, 0.0)), "at least two anchors are required"),
    (lambda: schedulers.PiecewiseLinearScheduler(), "at least two anchors are required"),
    (lambda: schedulers.TanhScheduler((0, 0.0), (5, 1.0), 0.0), "'eta' must be positive"),
    (lambda: schedulers.TanhScheduler((0, 0.0), (5, 1.0), -1.0), "'eta' must be positive"),
])
def test_scheduler_validation_errors_are_the_references(build, message):
    with pytest.raises(ValueError) as error:
        build()
    assert str(error.value) == message


# ------------------------------------------------------------------------------------------------ schedule hooks
def test_names_exports_and_training_only():
    parameter = cusrl.hook.HookParameterSchedule("entropy_loss", "weight", schedulers.StepScheduler(0.01))
    activation = cusrl.hook.HookActivationSchedule("entropy_loss", schedulers.LessThan(2))
    condition = cusrl.hook.ConditionalObjectiveActivation({"value_loss": cusrl.hook.EpochIndexCondition([0, 2])},
                                                          entropy_loss=cusrl.hook.EpochIndexCondition(0))
    stage = shared.stage(cusrl)
    capacity = cusrl.hook.OnPolicyBufferCapacitySchedule(schedulers.StepScheduler(4))
    assert parameter.name == "entropy_loss_weight_schedule" and activation.name == "entropy_loss_activation_schedule"
    assert condition.name == "conditional_objective_activation" and stage.name == "optimization_stage_aux"
    assert capacity.name == "on_policy_buffer_capacity_schedule"
    assert all(hook.training_only for hook in (parameter, activation, condition, capacity))
    assert list(condition.named_conditions) == ["value_loss", "entropy_loss"]
    assert isinstance(stage, HookComposite) and [hook.name for hook in stage] == ["state_estimation"]
    for name in ("ConditionalObjectiveActivation", "EpochIndexCondition", "HookActivationSchedule", "HookParameterSchedule",
                 "OptimizationStage"):
        assert name in cusrl.hook.__all__ and name in cusrl.hook.control.__all__
        assert getattr(cusrl.hook, name) is getattr(cusrl.hook.control, name)
    assert "OnPolicyBufferCapacitySchedule" in cusrl.hook.__all__ and "OnPolicyBufferCapacitySchedule" in cusrl.hook.on_policy.__all__


@pytest.mark.parametrize("build", [
    lambda: cusrl.hook.HookParameterSchedule("missing", "weight", schedulers.StepScheduler(0.01)),
    lambda: cusrl.hook.HookActivationSchedule("missing", schedulers.LessThan(2)),
])
def test_a_schedule_over_an_unknown_hook_is_refused_at_init(build):
    with pytest.raises(ValueError) as error:
        _agent(extra=[(build(), {})])
    assert str(error.value) == "No hook named 'missing' is registered"


def test_parameter_schedule_updates_the_mutable_and_records_floats():
    agent = _agent(1)
    entropy = agent.hook["entropy_loss"]
    assert entropy.weight == 0.01  # apply_schedule(0) ran at the end of construction
    agent.metrics.clear()
    agent.hook.apply_schedule(1)
    assert entropy.weight == 0.01 and agent.metrics.summary("Agent")["Agent/entropy_loss_weight"] == pytest.approx(0.01)
    agent.hook.apply_schedule(2)
    assert entropy.weight == 0.0
    agent.set_iteration(1)  # (the agent applies the schedules of the iteration it is set to)
    assert entropy.weight == 0.01
    # values that are no floats are applied and not recorded
    agent = _agent(extra=[(cusrl.hook.HookParameterSchedule("value_loss", "loss_clip", schedulers.StepScheduler(None, (1, 1))), {})])
    agent.metrics.clear()
    agent.hook.apply_schedule(1)
    assert agent.hook["value_loss"].loss_clip == 1 and not agent.metrics.summary("Agent")


def test_a_schedule_over_an_attribute_that_is_not_mutable_still_raises():
    hook = cusrl.hook.HookParameterSchedule("generalized_advantage_estimation", "recompute", schedulers.StepScheduler(True))
    with pytest.raises(ValueError, match="Attribute 'recompute' is not mutable on hook 'generalized_advantage_estimation'"):
        _agent(extra=[(hook, {})])  # (raised by the apply_schedule(0) that ends construction)


def test_activation_schedule_switches_the_hook_and_the_capture_signature_follows():
    from cusrl_amd.template.graphs import capture_signature

    agent = _agent(2)
    entropy = agent.hook["entropy_loss"]
    assert entropy.active
    before = capture_signature(agent)
    agent.hook.apply_schedule(1)
    assert entropy.active and capture_signature(agent) == before
    agent.hook.apply_schedule(2)
    assert not entropy.active and capture_signature(agent) != before
    assert "entropy_loss" not in [hook.name for hook in agent.hook.active_hooks()]
    agent.hook.apply_schedule(0)
    assert entropy.active and capture_signature(agent) == before


# ------------------------------------------------------------------------------------------------ conditional activation
class _Term(Hook):
    """An objective hook that counts its calls (the fake-hook pattern of tests/test_host_logic.py)."""

    def __init__(self, name):
        super().__init__()
        self.name_(name)
        self.calls = {"pre_objective": 0, "objective": 0}

    def pre_objective(self, metadata, batch):
        self.calls["pre_objective"] += 1

    def objective(self, metadata, batch):
        self.calls["objective"] += 1
        return {self.name: torch.zeros(())}


def _fake_agent(composite, **fields):
    agent = SimpleNamespace(inference_mode=False, device=torch.device("cpu"), fuse_objective=False, hook=composite, **fields)
    composite.pre_init(agent)
    return agent


def test_conditional_activation_flips_per_step_and_restores_in_post_update():
    seen = []

    def odd_minibatch(agent, metadata, batch):
        seen.append((agent, metadata["mini_batch_index"], batch))
        return metadata["mini_batch_index"] % 2 == 1

    a, b, c = _Term("a"), _Term("b").active_(False), _Term("c")
    control = cusrl.hook.ConditionalObjectiveActivation({"a": cusrl.hook.EpochIndexCondition(0)}, b=cusrl.hook.EpochIndexCondition([0, 1]),
                                                        c=odd_minibatch)
    composite = HookComposite([control, a, b, c])
    agent = _fake_agent(composite)
    assert control.eager_phases() == ("objective",)  # flips between minibatch steps: those steps stay out of capture
    composite.pre_update({})
    batch = {"x": 1}
    pattern = []
    for epoch in range(2):
        for minibatch in range(2):
            metadata = {"epoch_index": epoch, "mini_batch_index": minibatch}
            composite.pre_objective(metadata, batch)
            pattern.append((a.active, b.active, c.active))
            composite.objective(metadata, batch)
    # a: first epoch only; b: inactive before the update, stays off whatever its condition says; c: odd minibatches
    assert pattern == [(True, False, False), (True, False, True), (False, False, False), (False, False, True)]
    assert a.calls == {"pre_objective": 2, "objective": 2} and b.calls == {"pre_objective": 0, "objective": 0}
    assert c.calls == {"pre_objective": 2, "objective": 2}  # (switched on for the very step whose pre_objective flipped it)
    assert seen[0][0] is agent and seen[0][2] is batch and [entry[1] for entry in seen] == [0, 1, 0, 1]
    composite.post_update()
    assert (a.active, b.active, c.active) == (True, False, True)
    # an activity that changed between two updates is what the next update remembers
    a.active_(False), b.active_(True)
    composite.pre_update({})
    composite.pre_objective({"epoch_index": 0, "mini_batch_index": 1}, batch)
    assert (a.active, b.active, c.active) == (False, True, True)
    composite.post_update()
    assert (a.active, b.active, c.active) == (False, True, True)


def test_an_agent_with_conditional_activation_keeps_its_minibatch_steps_out_of_capture():
    from cusrl_amd.template.graphs import eager_phases

    assert eager_phases(_agent()) == set()
    agent = _agent(3)
    assert eager_phases(agent) == {"objective"} and not agent._graphable()
    order = [hook.name for hook in agent.hook]
    assert order.index("conditional_objective_activation") < order.index("value_loss")


# ------------------------------------------------------------------------------------------------ optimization stage
class _Regression(Hook):
    """A stage hook in plain torch: fits ``head(x)`` to ``y`` and records what the stage hands it."""

    def __init__(self):
        super().__init__()
        self.name_("regression")
        self.seen = []

    def init(self):
        self.register_module("head", torch.nn.Linear(2, 1))

    def pre_objective(self, metadata, batch):
        self.seen.append(("pre_objective", metadata.get("optimization_stage")))

    def objective(self, metadata, batch):
        self.seen.append(("objective", metadata.get("optimization_stage")))
        return {"regression_loss": (self.head(batch["x"]) - batch["y"]).square().mean()}

    def pre_optim(self, optimizer):
        self.seen.append(("pre_optim", optimizer))

    def post_optim(self):
        self.seen.append(("post_optim", None))

    def post_objective(self, metadata, batch):
        self.seen.append(("post_objective", metadata.get("optimization_stage")))


def _stage_agent(lr=0.1):
    regression = _Regression()
    stage = cusrl.hook.OptimizationStage("fit", [regression], cusrl.preset.AdamFactory(defaults={"lr": lr}))
    return _agent(extra=[(stage, {})]), stage, regression


def test_optimization_stage_runs_its_hooks_in_post_objective_with_its_own_optimizer():
    from cusrl_amd.hook.on_policy.fused import FusedPpoObjective
    from cusrl_amd.template.graphs import capture_signature, eager_phases

    agent, stage, regression = _stage_agent()
    assert agent.hook["optimization_stage_fit"] is stage and agent.hook["optimization_stage_fit.regression"] is regression
    assert eager_phases(agent) == {"objective"} and not agent._graphable()
    # the outer objective phase passes the stage by: no-ops, and the composition checks see a hook without an objective
    assert type(stage).objective is Hook.objective and type(stage).pre_optim is Hook.pre_optim and type(stage).post_optim is Hook.post_optim
    metadata, batch = {"epoch_index": 0}, {"x": torch.randn(16, 2), "y": torch.randn(16, 1)}
    stage.pre_objective(metadata, batch)
    assert stage.objective(metadata, batch) is None and regression.seen == []
    stage.pre_optim(agent.optimizer), stage.post_optim()
    assert regression.seen == []
    agent.device = torch.device("cuda")
    assert FusedPpoObjective.mode(agent.hook) == "fused"  # (asked of the composition only: nothing runs on the device here)
    agent.device = torch.device("cpu")
    # the stage optimizer: built over all of the agent's parameters, separate from the agent's own
    names = [name for group in stage.optimizer.param_groups for name in group["param_names"]]
    assert names == [name for name, _ in agent.named_parameters()] and "hook.optimization_stage_fit.regression.head.weight" in names
    assert stage.optimizer is not agent.optimizer and isinstance(stage.grad_scaler, torch.GradScaler)
    assert stage.grad_scaler.is_enabled() == agent.grad_scaler.is_enabled() is False
    # the children's mutables and flags are part of what a captured region is replayed under
    before = capture_signature(agent)
    regression.active_(False)
    assert capture_signature(agent) != before
    regression.active_(True)

    others = {name: param.detach().clone() for name, param in agent.named_parameters() if "regression" not in name}
    head = [param.detach().clone() for param in regression.head.parameters()]
    agent.metrics.clear()
    stage.post_objective(metadata, batch)
    name = "optimization_stage_fit"
    assert [entry[0] for entry in regression.seen] == ["pre_objective", "objective", "pre_optim", "post_optim", "post_objective"]
    assert [entry[1] for entry in regression.seen if entry[0] != "pre_optim"] == [name, name, None, name]
    assert regression.seen[2][1] is stage.optimizer and "optimization_stage" not in metadata
    assert all(not torch.equal(now, then) for now, then in zip(regression.head.parameters(), head))  # the stage stepped its hook
    for key, param in agent.named_parameters():  # ... and nothing the loss does not reach
        assert key not in others or torch.equal(param, others[key]), key
    first = agent.metrics.summary("Agent")["Agent/regression_loss"]
    for _ in range(50):
        stage.post_objective(metadata, batch)
    agent.metrics.clear()
    stage.post_objective(metadata, batch)
    assert agent.metrics.summary("Agent")["Agent/regression_loss"] < first  # (it does fit)
    # the stage's backward left gradients of its own on the parameters: the agent's next zero_grad re-attaches its flat buffer
    assert agent.flat_gradients is not None and not agent.flat_gradients.intact()
    agent._zero_grad()
    assert agent.flat_gradients.intact()


def test_optimization_stage_state_round_trips_through_the_agents_state_dict():
    agent, stage, regression = _stage_agent()
    batch = {"x": torch.randn(16, 2), "y": torch.randn(16, 1)}
    for _ in range(3):
        stage.post_objective({}, batch)
    state = copy.deepcopy(agent.state_dict())  # (as a checkpoint file would: torch's optimizers adopt the tensors they are handed)
    entry = state["hook"]["optimization_stage_fit"]
    assert set(entry) == {"regression", "optimizer", "grad_scaler"} and set(entry["regression"]) == {"head"}
    steps = [int(s["step"]) for s in entry["optimizer"]["state"].values()]
    assert steps and set(steps) == {3}

    other, other_stage, other_regression = _stage_agent()
    assert not other_stage.optimizer.state_dict()["state"]
    other.load_state_dict(state)
    loaded = other_stage.optimizer.state_dict()
    assert loaded["state"].keys() == entry["optimizer"]["state"].keys()
    for key, slot in entry["optimizer"]["state"].items():
        assert int(loaded["state"][key]["step"]) == 3
        assert torch.equal(loaded["state"][key]["exp_avg"], slot["exp_avg"]) and torch.equal(loaded["state"][key]["exp_avg_sq"], slot["exp_avg_sq"])
    assert other_stage.grad_scaler.state_dict() == entry["grad_scaler"]
    for mine, theirs in zip(other_regression.head.parameters(), regression.head.parameters()):
        assert torch.equal(mine, theirs)
    # both continue identically
    stage.post_objective({}, batch), other_stage.post_objective({}, batch)
    for mine, theirs in zip(other_regression.head.parameters(), regression.head.parameters()):
        assert torch.equal(mine, theirs)


def test_a_latent_reading_hook_does_not_fit_a_stage():
    """Why configuration 4 of the fixture uses StateEstimation: a hook that differentiates through the agent's own forward pass
    finds that graph freed by the agent's backward."""
    x = torch.randn(4, 2)
    layer, predictor = torch.nn.Linear(2, 2), torch.nn.Linear(2, 1)
    latent = layer(x).relu()
    latent.sum().backward()  # the agent's step
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        predictor(latent).square().mean().backward()  # the stage's


# ------------------------------------------------------------------------------------------------ buffer capacity
def test_buffer_capacity_schedule_sets_the_rollout_length_and_the_capacity():
    agent = _agent(5)
    assert agent.num_steps_per_update == 4 and agent.buffer.capacity == 4 and agent.buffer_capacity == 4
    version = agent.buffer.layout_version
    agent.hook.apply_schedule(1)
    assert agent.num_steps_per_update == 4 and agent.buffer.capacity == 4 and agent.buffer.layout_version == version
    agent.hook.apply_schedule(2)
    assert agent.num_steps_per_update == 6 and agent.buffer.capacity == 6 and agent.buffer_capacity == 6
    assert agent.buffer.layout_version != version and not agent.buffer.storage  # emptied: captured regions see another layout
    version = agent.buffer.layout_version
    agent.hook.apply_schedule(3)
    assert agent.buffer.capacity == 6 and agent.buffer.layout_version == version  # held: nothing moves
    from cusrl_amd.template.agent import Agent

    assert [Agent.step(agent, None, None, None, None) for _ in range(6)] == [False] * 5 + [True]  # an update every 6 steps now


# ------------------------------------------------------------------------------------------------ re-capture hysteresis
def test_a_signature_that_keeps_moving_keeps_a_region_eager_until_it_holds():
    from cusrl_amd.template.graphs import _Settling

    agent = SimpleNamespace(iteration=0)
    settling = _Settling(agent)
    assert settling.holds("a") and settling.holds("a")  # first sight is no change
    agent.iteration = 1
    assert not settling.holds("b") and not settling.repeated  # changed in this iteration: eager for the rest of it ...
    assert not settling.holds("b")
    agent.iteration = 2
    assert settling.holds("b")  # ... captured in the first iteration that begins under the same signature
    agent.iteration = 3
    assert not settling.holds("c") and not settling.repeated  # (the change before was two iterations ago)
    agent.iteration = 4
    assert not settling.holds("d") and settling.repeated  # a change in the iteration after a change: a schedule
    agent.iteration = 5
    assert not settling.holds("e") and settling.repeated
    agent.iteration = 6
    assert settling.holds("e")


def test_the_fixture_names_the_parameters_this_package_names(golden):
    g = golden("control_hooks")
    for config in shared.CONFIGS:
        agent = _agent(config)
        assert [name for name, _ in agent.named_parameters()] == [str(name) for name in g[f"c{config}_param_names"]], config
