"""Regenerate ``control_hooks.npz``: the reference's schedulers (cusrl/utils/scheduler.py) evaluated on iterations -1..12, and
four-iteration update traces of a tiny `ppo` agent on the dummy environment under each of the control hooks
(cusrl/hook/control, cusrl/hook/on_policy/buffer_schedule.py), recorded on CPU in the format of
make_symmetric_actor_golden.make_update_trace: the initial parameters, every iteration's buffer as its update finds it, the
objectives of every minibatch step and the parameters after every update.

    python tests/golden/make_control_hooks_golden.py
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
ITERATIONS = 4
ENVS, OBS, ACT = 8, 6, 3
FACTORY_KWARGS = dict(num_steps_per_update=4, sampler_epochs=2, sampler_mini_batches=2)
SCHEDULER_ITERATIONS = list(range(-1, 13))
TERMS = ("value_loss", "surrogate_loss", "entropy_loss")


def scheduler_cases(module):
    """name -> scheduler; anchors at steps 2 and 9, so that -1..12 covers before, both anchors, between and after (restated for this
    package in tests/_control_hooks.py)."""
    return {
        "less_than": module.LessThan(2),
        "not_less_than": module.NotLessThan(9),
        "step": module.StepScheduler(0.01, (2, 0.5), (9, 0.0)),
        "piecewise": module.PiecewiseLinearScheduler((2, 0.01), (5, 0.3), (9, 0.0)),
        "piecewise_two": module.PiecewiseLinearScheduler((2, 1.0), (9, 0.1)),
        "cosine": module.CosineAnnealingScheduler((2, 0.01), (9, 0.7)),
        "tanh_half": module.TanhScheduler((2, 0.01), (9, 0.7), 0.5),
        "tanh_three": module.TanhScheduler((2, 0.7), (9, 0.01), 3),
    }


def control_hooks(cusrl, config: int, state_estimation=None):
    """``[(hook, where)]`` of configuration ``config`` (1..5), restated for this package in tests/_control_hooks.py.
    ``state_estimation``: the class to build the stage's hook from (a patched subclass, see make_traces)."""
    hook, scheduler = cusrl.hook, cusrl.utils.scheduler
    if config == 1:
        return [(hook.HookParameterSchedule("entropy_loss", "weight", scheduler.StepScheduler(0.01, (2, 0.0))), {})]
    if config == 2:
        return [(hook.HookActivationSchedule("entropy_loss", scheduler.LessThan(2)), {})]
    if config == 3:
        return [(hook.ConditionalObjectiveActivation(entropy_loss=hook.control.EpochIndexCondition(0)), {"before": "value_loss"})]
    if config == 4:
        # ReturnPrediction does not fit a stage: it reads the actor's latent of the agent's own forward pass, whose autograd graph
        # the agent's backward has freed by the time the stage differentiates.  StateEstimation runs its own estimator on the
        # batch; here it learns the next observation from the observation (the dummy environment has no privileged state).
        estimation = (state_estimation or hook.StateEstimation)(cusrl.Mlp.Factory([12]), target_name="next_observation", weight=0.5)
        stage = hook.OptimizationStage("aux", [estimation], cusrl.preset.AdamFactory(defaults={"lr": 1e-3}))
        return [(stage, {"before": "on_policy_statistics"})]
    if config == 5:
        return [(hook.OnPolicyBufferCapacitySchedule(scheduler.StepScheduler(4, (2, 6))), {})]
    raise AssertionError(config)


def make_schedulers(cusrl, out):
    out["scheduler_iterations"] = np.array(SCHEDULER_ITERATIONS)
    cases = scheduler_cases(cusrl.utils.scheduler)
    out["scheduler_names"] = np.array(list(cases))
    for name, scheduler in cases.items():
        values = [scheduler(iteration) for iteration in SCHEDULER_ITERATIONS]
        out["scheduler/" + name] = np.array(values, dtype=bool if isinstance(values[0], bool) else np.float64)


def make_traces(cusrl, out):
    from cusrl.testing.environment import DummyTorchEnvironment  # noqa: PLC0415

    class StateEstimation(cusrl.hook.StateEstimation):
        """(as in make_privileged_golden.py: the reference stores no ``estimator_memory`` leaf for a feed-forward estimator and
        then looks it up with ``batch["estimator_memory"]``: the lookup is given its None, nothing else changes)"""

        def objective(self, metadata, batch):
            batch.setdefault("estimator_memory", None)
            return super().objective(metadata, batch)

    out["iterations"] = np.array(ITERATIONS)
    out["factory_keys"] = np.array(list(FACTORY_KWARGS))
    out["factory_vals"] = np.array([float(v) for v in FACTORY_KWARGS.values()])
    out["shape"] = np.array([ENVS, OBS, ACT])
    for config in range(1, 6):
        torch.manual_seed(11)
        env = DummyTorchEnvironment(num_instances=ENVS, observation_dim=OBS, action_dim=ACT, reward_dim=1)
        underlying = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(16, 16), critic_hidden_dims=(16, 16), **FACTORY_KWARGS).to_underlying()
        extra = control_hooks(cusrl, config, StateEstimation)
        for hook, where in extra:
            underlying.register_hook(hook, **where)
        agent = underlying(env.spec)
        trace = {"objectives": [], "stage": []}
        outer = agent.hook.objective

        def wrapped(metadata, batch, _outer=outer):
            result = _outer(metadata, batch)
            trace["objectives"].append(np.array([result[key].item() if key in result else np.nan for key in TERMS], dtype=np.float32))
            return result

        agent.hook.objective = wrapped
        if config == 4:
            child = extra[0][0]["state_estimation"]
            inner = child.objective

            def staged(metadata, batch, _inner=inner):
                assert metadata["optimization_stage"] == "optimization_stage_aux"
                result = _inner(metadata, batch)
                trace["stage"].append(np.float32(result["state_estimation_loss"].item()))
                return result

            child.objective = staged

        p = f"c{config}_"
        state0 = {name: np_(param) for name, param in agent.named_parameters()}
        out[p + "param_names"] = np.array(list(state0))
        for name, value in state0.items():
            out[p + "param0/" + name] = value
        observation, state, _ = env.reset()
        step = 0
        for iteration in range(ITERATIONS):
            while True:
                action = agent.act(observation, state)
                observation, state, reward, terminated, truncated, _ = env.step(action)
                ready = agent.step(observation, reward, terminated, truncated, state)
                step += 1
                if ready:
                    break
            # (next_value / advantage / return are what the update writes: stale leftovers of the previous one are not inputs)
            buffer_in = {k: np_(v) for k, v in agent.buffer.storage.items() if k not in ("next_value", "advantage", "return")}
            seen, staged_seen = len(trace["objectives"]), len(trace["stage"])
            torch.manual_seed(99 + iteration)  # generator state at the update boundary
            metrics = agent.update()
            q = f"{p}{iteration}_"
            out[q + "buffer_keys"] = np.array(list(buffer_in))
            for k, v in buffer_in.items():
                out[q + "buffer_in/" + k] = v
            out[q + "objectives"] = np.stack(trace["objectives"][seen:])
            if config == 4:
                out[q + "stage_objectives"] = np.array(trace["stage"][staged_seen:], dtype=np.float32)
            out[q + "params_after"] = np_(torch.cat([param.detach().reshape(-1) for _, param in agent.named_parameters()]))
            out[q + "metric_keys"] = np.array(list(metrics.keys()))
            out[q + "metric_vals"] = np.array(list(metrics.values()), dtype=np.float64)
            capacity = next(iter(buffer_in.values())).shape[0]
            print(f"config {config}, iteration {iteration}: capacity {capacity}, {len(trace['objectives']) - seen} train steps, "
                  f"entropy term in {int(np.isfinite(out[q + 'objectives'][:, 2]).sum())} of them, leaves {list(buffer_in)}")


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_schedulers(cusrl, out)
    make_traces(cusrl, out)
    np.savez_compressed(HERE / "control_hooks.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("control_hooks.npz:", len(out), "arrays,", (HERE / "control_hooks.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
