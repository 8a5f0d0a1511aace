"""The control hooks on an MI355X: the reference's recorded four-iteration traces under each of the five configurations (golden
``control_hooks.npz``), training under capture against the eager run bit for bit, the schedule hooks against a twin driven by
hand, and what the captured regions do when a schedule moves their signature (template/graphs.py ``_Settling``)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _control_hooks as shared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TERMS = ("value_loss", "surrogate_loss", "entropy_loss")
STEP_REGION = "GraphedTrainStep._whole_step"
ROLLOUT_STEP_REGION = "GraphedRolloutStep._body"
WHOLE_ROLLOUT_REGION = "GraphedRolloutStep.run_rollout.<locals>.<lambda>"
UPDATE_REGION = "GraphedEpochs.run.<locals>.<lambda>"
STATISTICS_REGION = "OnPolicyStatistics._post_update_replayed.<locals>.region"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _host(t):
    return t.detach().cpu().numpy()


def _flat(agent):
    return torch.cat([param.detach().reshape(-1) for _, param in agent.named_parameters()]).clone()


# ------------------------------------------------------------------------------------------------ the reference's traces
@pytest.mark.parametrize("config", shared.CONFIGS)
def test_four_iterations_replay_the_reference_trace(cusrl, golden, config):
    """Every iteration from the recorded buffer: the objectives of every minibatch step and the parameters after the update, held
    to the bounds of the existing update-trace replays (tests/test_agent_gpu.py: objectives rtol 2e-5, parameters rtol 1e-4)."""
    g = golden("control_hooks")
    agent = shared.factory(cusrl, config, DEV)(cusrl.EnvironmentSpec(shared.OBS, shared.ACT, num_instances=shared.ENVS, device=DEV))
    p = f"c{config}_"
    named = dict(agent.named_parameters())
    assert list(named) == [str(name) for name in g[p + "param_names"]]
    with torch.no_grad():
        for name, param in named.items():
            param.copy_(torch.from_numpy(g[f"{p}param0/{name}"]).to(DEV))
    agent.sampler.permutation_device = "cpu"  # CPU-generator permutations reproduce the CPU reference's stream
    agent.hook["on_policy_statistics"].sampler.permutation_device = "cpu"
    objectives, staged = [], []
    outer = agent.hook.objective

    def wrapped(metadata, batch):
        result = outer(metadata, batch)
        objectives.append([float(result[key].detach()) if key in result else float("nan") for key in TERMS])
        return result

    agent.hook.objective = wrapped
    if config == 4:
        child = agent.hook["optimization_stage_aux.state_estimation"]
        inner = child.objective

        def stage_objective(metadata, batch):
            assert metadata["optimization_stage"] == "optimization_stage_aux"
            result = inner(metadata, batch)
            staged.append(float(result["state_estimation_loss"].detach()))
            return result

        child.objective = stage_objective
    for iteration in range(int(g["iterations"])):
        q = f"{p}{iteration}_"
        leaves = {str(k): g[f"{q}buffer_in/{k}"] for k in g[q + "buffer_keys"]}
        capacity = leaves["observation"].shape[0]
        assert agent.num_steps_per_update == agent.buffer.capacity == capacity == (6 if config == 5 and iteration >= 2 else 4)
        for t in range(capacity):
            step = {k: torch.from_numpy(np.ascontiguousarray(v[t])).to(DEV) for k, v in leaves.items() if not k.startswith("action_dist.")}
            step["action_dist"] = {key: torch.from_numpy(leaves["action_dist." + key][t]).to(DEV) for key in ("mean", "std")}
            agent.buffer.push(step)
        assert agent.buffer.full and agent.buffer.cursor == 0
        seen, staged_seen = len(objectives), len(staged)
        torch.manual_seed(99 + iteration)
        metrics = agent.update()
        got, expected = np.array(objectives[seen:], dtype=np.float32), g[q + "objectives"]
        print(f"config {config}, iteration {iteration}: objectives max |difference| {np.nanmax(np.abs(got - expected)):.3e}, "
              f"parameters {np.abs(_host(_flat(agent)) - g[q + 'params_after']).max():.3e}")
        assert np.array_equal(np.isnan(got), np.isnan(expected)), "the entropy term is present in other steps than the reference's"
        np.testing.assert_allclose(got, expected, rtol=2e-5, atol=1e-6)
        if config == 4:
            np.testing.assert_allclose(np.array(staged[staged_seen:], dtype=np.float32), g[q + "stage_objectives"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(_host(_flat(agent)), g[q + "params_after"], rtol=1e-4, atol=2e-6)
        reference = dict(zip((str(k) for k in g[q + "metric_keys"]), g[q + "metric_vals"]))
        assert ("Agent/entropy_loss" in metrics) == ("Agent/entropy_loss" in reference)
        for key in ("Agent/entropy_loss_weight", "Agent/state_estimation_loss"):
            assert (key in metrics) == (key in reference), key
            if key in reference:
                assert metrics[key] == pytest.approx(reference[key], rel=1e-3, abs=1e-6), key


# ------------------------------------------------------------------------------------------------ training runs
def _train(cusrl, hooks, compile, iterations=4, before_iteration=None, seed=21, reseed=False):
    """``iterations`` rollouts + updates of the tiny agent through the Trainer; returns the trainer, the parameters after every
    iteration, every iteration's log, the buffer's capacity after every iteration and the capture counts after every iteration.
    ``compile``: False, True, or ``"eager"`` — the compile=True agent with its minibatch steps kept out of capture by a hook that declares
    the objective phase eager and with the host-driven rollout loop (as tests/test_captured_rollout.py compares): the same
    kernels, optimizer and streams as the captured run, issued by Python every time."""
    from cusrl_amd.template.graphs import _Capture

    eager = compile == "eager"
    if eager:
        # (ConditionalObjectiveActivation without conditions does nothing but declare the objective phase eager; a hook class of the
        # test's own would also switch off what the package only does among its own hooks, ValueComputation's deferred pass)
        hooks, compile = list(hooks) + [(cusrl.hook.ConditionalObjectiveActivation().name_("eager_objective"), {})], True
    cusrl.set_global_seed(seed)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=shared.ENVS, observation_dim=shared.OBS, action_dim=shared.ACT, device=DEV)
    factory = shared.factory(cusrl, None, None, hooks, compile=compile, optimizer_kwargs={"capturable": True, "fused": True})
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    if eager:
        trainer.capture_rollout = False
    if reseed:  # (a composition whose construction draws more initial weights: the run itself starts from the same generator state)
        cusrl.set_global_seed(seed)
    agent = trainer.agent
    params, logs, capacities, counts = [], [], [], []
    observation, state, _ = env.reset(randomize_episode_progress=True)
    for iteration in range(iterations):
        if before_iteration is not None:
            before_iteration(agent, iteration)
        observation, state = trainer._rollout_and_update(observation, state)
        trainer.iteration += 1
        logs.append(dict(trainer.last_info))
        params.append(_flat(agent))
        capacities.append({leaf.shape[0] for leaf in agent.buffer.storage.values()})
        counts.append(dict(_Capture.counts))
    return trainer, params, logs, capacities, counts


def _hooks(cusrl, config):
    return shared.control_hooks(cusrl, config)


def _assert_same_bits(a, b):
    assert len(a) == len(b)
    for iteration, (mine, theirs) in enumerate(zip(a, b)):
        assert torch.equal(mine, theirs), f"iteration {iteration}: {(mine - theirs).abs().max():.3e}"


@pytest.fixture(scope="module")
def runs(cusrl):
    """Configurations 1, 2, 3 and 5 from the same seed: under capture, the same agent issued eagerly, and compile=False."""
    return {(config, compile): _train(cusrl, _hooks(cusrl, config), compile) for config in (1, 2, 3, 5) for compile in (True, "eager", False)}


@pytest.mark.parametrize("config", [1, 2, 3, 5])
def test_training_under_capture_is_bit_identical_to_eager(cusrl, runs, config):
    """Replayed against issued: the compile=True agent with its graphs, and the same agent with its minibatch steps and its rollout loop issued by
    Python — bit for bit after every iteration.  (Against compile=False the PLAIN `ppo` agent, without any control hook and with every capture
    switched off, already differs in the last bits at this shape — 3.7e-9 after iteration 1 —, so that pair is held to what
    tests/test_agent_gpu.py holds it to: rtol 1e-4, atol 1e-5.)"""
    captured, eager, plain = runs[config, True], runs[config, "eager"], runs[config, False]
    agent = captured[0].agent
    assert agent._graphed_act is not None and captured[0]._graphed_rollout is not None  # (it did go through the captured paths)
    assert bool(agent._graphed_steps) == (config != 3)  # conditional activation: the minibatch steps stay eager
    assert not eager[0].agent._graphed_steps and eager[0]._graphed_rollout is None
    _assert_same_bits(captured[1], eager[1])
    assert not torch.equal(captured[1][0], captured[1][-1])
    for mine, theirs in zip(captured[1], plain[1]):
        assert torch.allclose(mine, theirs, rtol=1e-4, atol=1e-5), (mine - theirs).abs().max()
    if config == 5:
        # (the schedule of iteration 2 is applied at the end of iteration 1, which empties the buffer)
        assert captured[3] == eager[3] == plain[3] == [{4}, set(), {6}, {6}]
        assert agent.num_steps_per_update == agent.buffer.capacity == 6


def test_parameter_schedule_equals_a_twin_driven_by_hand(cusrl, runs):
    scheduler = cusrl.utils.StepScheduler(0.01, (2, 0.0))

    def by_hand(agent, iteration):
        assert "entropy_loss_weight_schedule" not in [hook.name for hook in agent.hook]
        agent.hook["entropy_loss"].update_attribute("weight", scheduler(iteration))

    for compile in (True, "eager", False):
        twin = _train(cusrl, [], compile, before_iteration=by_hand)
        _assert_same_bits(runs[1, compile][1], twin[1])
        assert twin[0].agent.hook["entropy_loss"].weight == runs[1, compile][0].agent.hook["entropy_loss"].weight == 0.0
    logs = runs[1, True][2]
    assert [log["Agent/entropy_loss_weight"] for log in logs] == pytest.approx([0.01, 0.0, 0.0, 0.0])  # (recorded for the NEXT iteration)
    assert [log["Agent/entropy_loss"] != 0.0 for log in logs] == [True, True, False, False]


def test_activation_schedule_equals_a_twin_driven_by_hand(cusrl, runs):
    scheduler = cusrl.utils.LessThan(2)

    def by_hand(agent, iteration):
        agent.hook["entropy_loss"].active_(scheduler(iteration))

    for compile in (True, "eager", False):
        twin = _train(cusrl, [], compile, before_iteration=by_hand)
        _assert_same_bits(runs[2, compile][1], twin[1])
        logs = runs[2, compile][2]
        # the term is absent from the iterations in which the hook is off — not recorded as zero
        assert ["Agent/entropy_loss" in log for log in logs] == [True, True, False, False], compile
        assert all("Agent/surrogate_loss" in log and "Agent/value_loss" in log for log in logs)


def test_a_weight_that_moves_every_iteration_does_not_recapture_every_iteration(cusrl):
    from cusrl_amd.template.graphs import _Capture

    def hooks():
        return [(cusrl.hook.HookParameterSchedule("entropy_loss", "weight", cusrl.utils.PiecewiseLinearScheduler((0, 0.01), (8, 0.0))), {})]

    before = dict(_Capture.counts)
    trainer, params, logs, _, counts = _train(cusrl, hooks(), True, iterations=6)
    moved = [{key: value - before.get(key, 0) for key, value in count.items() if value != before.get(key, 0)} for count in counts]
    print("captures by region after every iteration:", moved)
    agent = trainer.agent
    # (an iteration's log holds the weight its update scheduled for the NEXT one; iteration 0's also holds construction's)
    assert [log["Agent/entropy_loss_weight"] for log in logs[1:]] == pytest.approx([0.01 * (1 - k / 8) for k in range(2, 7)])
    # every minibatch step is captured once — in iteration 0, before the weight first moves — and runs eagerly from then on
    # (without the hysteresis: once more in every later iteration, 2 + 2 * 5 captures)
    steps = list(agent._graphed_steps.values())
    assert len(steps) == 2 and moved[-1].get(STEP_REGION, 0) <= len(steps)
    assert moved[0].get(STEP_REGION, 0) == moved[-1].get(STEP_REGION, 0)  # nothing after iteration 0
    assert all(step.state == 1 for step in steps)
    # the env steps: captured when they are warm (iteration 2), eager once the signature has moved twice in a row
    assert moved[-1].get(ROLLOUT_STEP_REGION, 0) <= 4 and moved[-1].get(WHOLE_ROLLOUT_REGION, 0) == 0
    assert moved[-1] == moved[2], "a region was captured again after iteration 2"
    eager = _train(cusrl, hooks(), "eager", iterations=6)
    _assert_same_bits(params, eager[1])


def test_a_new_capacity_recaptures_once_and_not_again_while_it_holds(cusrl):
    """Configuration 5, continued with the capacity held.  Within the fixture's four iterations — two of each capacity — the
    regions of the update that are sized by the rollout length (the minibatch steps, the whole-update graph on top of them, the
    statistics pass) are captured once per capacity, twice in all.  A rollout's own step graphs need three rollouts of a layout
    (one host-driven, one eager warm-up, then the capture: template/trainer.py, graphs.py), so those of capacity 4 never come to
    be and those of capacity 6 follow in iterations 3 and 4, the whole-rollout graph in iteration 5 and the value pass behind it.
    Every graph is captured exactly once, and nothing is captured in the last three iterations."""
    from cusrl_amd.template.graphs import _Capture

    before = dict(_Capture.counts)
    trainer, params, _, capacities, counts = _train(cusrl, _hooks(cusrl, 5), True, iterations=10)
    moved = [{key: value - before.get(key, 0) for key, value in count.items() if value != before.get(key, 0)} for count in counts]
    print("captures by region after every iteration:", moved)
    assert capacities == [{4}, set()] + [{6}] * 8  # the leaves after iteration 2 show capacity 6
    agent, graphed = trainer.agent, trainer._graphed_rollout
    assert {tuple(leaf.shape[:2]) for leaf in agent.buffer.storage.values()} == {(6, shared.ENVS)}
    # the minibatch steps: one graph per slot and batch size, 2 of 16 rows (capacity 4) and 2 of 24 rows, each captured once
    assert sorted(key[2] for key in agent._graphed_steps) == [16, 16, 24, 24]
    assert [m.get(STEP_REGION, 0) for m in moved[:4]] == [2, 2, 4, 4] and moved[-1][STEP_REGION] == 4
    # once per distinct capacity, twice in all over the four iterations: the whole-update graph and the statistics pass
    for region in (UPDATE_REGION, STATISTICS_REGION):
        assert [m.get(region, 0) for m in moved[:4]] == [0, 1, 1, 2] and moved[-1][region] == 2, region
    # the env steps: one graph per buffer cursor of the new capacity, each captured once; then the whole rollout, once
    assert graphed.captured == 6 and moved[-1][ROLLOUT_STEP_REGION] == 6 and moved[-1][WHOLE_ROLLOUT_REGION] == 1
    assert len(graphed.rollouts) == 1 and graphed.rollout_replays >= 3
    assert moved[-1] == moved[-2] == moved[-3] == moved[-4], "a region was captured again while the capacity held"
    eager = _train(cusrl, _hooks(cusrl, 5), "eager", iterations=10)
    _assert_same_bits(params, eager[1])


# ------------------------------------------------------------------------------------------------ the stage optimizer
def test_the_stage_optimizer_stays_separate(cusrl):
    from cusrl_amd.utils.flat_optimizer import FlatAdam

    def with_stage(lr):
        return [(shared.stage(cusrl, lr), {"before": "on_policy_statistics"})]

    def split(agent, flat):
        sizes = [(name, param.numel()) for name, param in agent.named_parameters()]
        parts, offset = {"stage": [], "agent": []}, 0
        for name, size in sizes:
            parts["stage" if "optimization_stage_aux" in name else "agent"].append(flat[offset:offset + size])
            offset += size
        return {key: torch.cat(value) if value else None for key, value in parts.items()}

    plain = _train(cusrl, [], False, reseed=True)
    frozen = _train(cusrl, with_stage(0.0), False, reseed=True)
    stage = frozen[0].agent.hook["optimization_stage_aux"]
    assert isinstance(frozen[0].agent.flat_optimizer, FlatAdam) and isinstance(stage.optimizer, torch.optim.Adam)
    assert stage.optimizer is not frozen[0].agent.optimizer and int(next(iter(stage.optimizer.state.values()))["step"]) == 4 * 4
    initial = None
    for iteration, (with_, without) in enumerate(zip(frozen[1], plain[1])):
        parts = split(frozen[0].agent, with_)
        # a stage whose learning rate is 0: actor and critic are stepped by the agent's own optimizer exactly as without the stage
        assert torch.equal(parts["agent"], without), f"iteration {iteration}: {(parts['agent'] - without).abs().max():.3e}"
        initial = parts["stage"] if initial is None else initial
        assert torch.equal(parts["stage"], initial)  # ... and the agent's optimizer never moves the stage's parameters
    assert "Agent/state_estimation_loss" in frozen[2][-1]
    trained = _train(cusrl, with_stage(1e-3), False, reseed=True)
    parts = [split(trained[0].agent, flat) for flat in trained[1]]
    assert not torch.equal(parts[0]["stage"], initial) and not torch.equal(parts[-1]["stage"], parts[0]["stage"])
    # the stage's loss reaches its estimator only: actor and critic still train exactly as without it
    _assert_same_bits([part["agent"] for part in parts], plain[1])
    assert trained[2][-1]["Agent/state_estimation_loss"] < trained[2][0]["Agent/state_estimation_loss"]
    # under compile=True the stage keeps the minibatch steps eager while the rollout is captured: the same bits as with the
    # host-driven rollout loop
    captured = _train(cusrl, with_stage(1e-3), True, reseed=True)
    assert not captured[0].agent._graphed_steps and captured[0]._graphed_rollout is not None and captured[0]._graphed_rollout.captured
    _assert_same_bits(captured[1], _train(cusrl, with_stage(1e-3), "eager", reseed=True)[1])
