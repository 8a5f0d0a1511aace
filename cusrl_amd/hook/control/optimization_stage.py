"""A second optimization pass per minibatch step with hooks and an optimizer of its own (counterpart of
cusrl/hook/control/optimization_stage.py).

Capture policy: the nested pass differentiates a loss and steps a torch optimizer from inside ``post_objective`` — a backward
through ``Tensor.backward`` and an optimizer whose step counter lives on the host, neither of which a replayed hipGraph would
repeat.  The stage declares the objective phase eager (``Hook.eager_phases``): the minibatch steps of an agent with a stage run
hook by hook.  The stage optimizer stays what its factory builds; it is never folded into the agent's flat gradient buffer,
flat Adam step or ``StepPlan`` (template/actor_critic.py), which keep serving the agent's own optimizer."""

from __future__ import annotations

from collections.abc import Iterable

import torch

from cusrl_amd.template.actor_critic import HookList
from cusrl_amd.template.hook import Hook, HookComposite
from cusrl_amd.template.optimizer import OptimizerFactory
from cusrl_amd.utils.distributed import reduce_gradients

__all__ = ["OptimizationStage"]


class OptimizationStage(HookComposite):
    """Runs ``stage_hooks`` through their own ``pre_objective -> objective -> pre_optim -> post_optim -> post_objective`` cycle
    behind the agent's, with a separate optimizer step in between.  Outside the objective phase (``pre_act``, ``post_step``,
    ``pre_update``, ...) the stage hooks take part like any other hook.  During the nested pass they see
    ``metadata | {"optimization_stage": <name of this hook>}``.

    Args:
        stage_name (str):
            Suffix of the hook's name, ``optimization_stage_{stage_name}``.
        stage_hooks (Iterable[Hook]):
            Hooks of the nested pass.
        optimizer_factory (OptimizerFactory):
            Builds the stage optimizer over ``agent.named_parameters()`` (narrow it with ``param_filter``).
    """

    # the outer objective phase passes the stage by: literally the base class's no-ops, so that the composition checks that ask
    # "does this hook define an objective / touch the gradients" (FusedPpoObjective.mode, plan_step) answer no
    pre_objective = Hook.pre_objective
    objective = Hook.objective
    pre_optim = Hook.pre_optim
    post_optim = Hook.post_optim

    def __init__(self, stage_name: str, stage_hooks: Iterable[Hook], optimizer_factory: OptimizerFactory):
        self.stage_name = stage_name
        self.stage_hooks = HookList.coerce(tuple(stage_hooks))
        self.optimizer_factory = optimizer_factory
        super().__init__(self.stage_hooks)
        self.name_(f"optimization_stage_{stage_name}")

        # Runtime attributes
        self.optimizer: torch.optim.Optimizer
        self.grad_scaler: torch.GradScaler

    @property
    def objective_draws_random(self) -> bool:
        return any(hook._active and hook.objective_draws_random for hook in self)

    @property
    def step_draws_random(self) -> bool:
        return any(hook._active and hook.step_draws_random for hook in self)

    def eager_phases(self) -> tuple[str, ...]:
        phases = {"objective"}
        for hook in self:
            if hook._active:
                phases |= set(hook.eager_phases())
        return tuple(sorted(phases))

    def collective_phases(self) -> tuple[str, ...]:
        phases: set[str] = set()
        for hook in self:
            if hook._active:
                phases |= set(hook.collective_phases())
        return tuple(sorted(phases))

    def post_init(self):
        self.register_stateful("optimizer", self.optimizer_factory(self.agent.named_parameters()))
        self.register_stateful("grad_scaler", torch.GradScaler(device=self.agent.device.type, enabled=self.agent.grad_scaler_enabled))
        super().post_init()

    def post_objective(self, metadata, batch):
        agent = self.agent
        stage_metadata = dict(metadata) | {"optimization_stage": self.name}
        HookComposite.pre_objective(self, stage_metadata, batch)
        with agent.autocast():
            objectives = HookComposite.objective(self, stage_metadata, batch)
        if objectives is not None:
            # the agent's gradients have been consumed by its own step; its flat buffer's views are put back by the agent's next
            # zero_grad (FlatGradients.intact / attach), so this backward never writes into that buffer
            self.optimizer.zero_grad()
            self.grad_scaler.scale(objectives.loss()).backward()
            self.grad_scaler.unscale_(self.optimizer)
            reduce_gradients(self.optimizer)
            HookComposite.pre_optim(self, self.optimizer)
            self.grad_scaler.step(self.optimizer)
            self.grad_scaler.update()
            HookComposite.post_optim(self)
            agent.record(**objectives)
        super().post_objective(stage_metadata, batch)
