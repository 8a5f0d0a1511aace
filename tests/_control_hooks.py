"""Shared by the control-hook tests (CPU and GPU): the scheduler cases and the five hook configurations of golden
``control_hooks.npz`` (tests/golden/make_control_hooks_golden.py), restated for this package."""

from __future__ import annotations

ENVS, OBS, ACT = 8, 6, 3
HIDDEN = (16, 16)
CONFIGS = (1, 2, 3, 4, 5)


def scheduler_cases(module):
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


def stage(cusrl, lr: float = 1e-3):
    """Configuration 4's stage.  StateEstimation, not ReturnPrediction: the latter reads the actor's latent of the agent's own
    forward pass, whose autograd graph the agent's backward has freed by the time a stage differentiates."""
    estimation = cusrl.hook.StateEstimation(cusrl.Mlp.Factory([12]), target_name="next_observation", weight=0.5)
    return cusrl.hook.OptimizationStage("aux", [estimation], cusrl.preset.AdamFactory(defaults={"lr": lr}))


def control_hooks(cusrl, config: int):
    """``[(hook, where)]`` of configuration ``config``."""
    hook, scheduler = cusrl.hook, cusrl.utils.scheduler
    if config == 1:
        return [(hook.HookParameterSchedule("entropy_loss", "weight", scheduler.StepScheduler(0.01, (2, 0.0))), {})]
    if config == 2:
        return [(hook.HookActivationSchedule("entropy_loss", scheduler.LessThan(2)), {})]
    if config == 3:
        return [(hook.ConditionalObjectiveActivation(entropy_loss=hook.EpochIndexCondition(0)), {"before": "value_loss"})]
    if config == 4:
        return [(stage(cusrl), {"before": "on_policy_statistics"})]
    if config == 5:
        return [(hook.OnPolicyBufferCapacitySchedule(scheduler.StepScheduler(4, (2, 6))), {})]
    raise AssertionError(config)


def factory(cusrl, config: int | None, device, extra=(), **overrides):
    """The tiny `ppo` agent factory of the fixture (8 envs x 6 obs x 3 act, T = 4, Mlp (16, 16), 2 epochs x 2 minibatches) with the
    hooks of ``config`` (None: none) and ``extra``."""
    kwargs = dict(num_steps_per_update=4, sampler_epochs=2, sampler_mini_batches=2, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN,
                  device=device)
    kwargs.update(overrides)
    underlying = cusrl.preset.PpoAgentFactory(**kwargs).to_underlying()
    for hook, where in (control_hooks(cusrl, config) if config is not None else []) + list(extra):
        underlying.register_hook(hook, **where)
    return underlying
