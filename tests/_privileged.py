"""Shared by the privileged-information tests (CPU and GPU): the hooks outside an agent on the seeded inputs of golden
``privileged.npz`` (tests/golden/make_privileged_golden.py), and the three compositions of its update traces."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

OBS, ACT, STATE, VALUE = 16, 8, 7, 1
# the reference was given the reversed slice as the list of its columns (torch refuses negative steps); here it is the slice
INDEX_FORMS = {"slice": slice(1, 6, 2), "list": [5, 0, 5], "reversed": slice(None, None, -1)}
CASES = ([(hook, form) for form in INDEX_FORMS for hook in ("estimation", "state_prediction", "next_state_prediction")]
         + [("return_prediction", "return"), ("return_prediction", "value"), ("distillation", None)])
AUX_KEYS = {"pa": ("state_estimation_loss",), "pb": ("state_prediction_loss", "return_prediction_loss"),
            "pc": ("next_state_prediction_loss", "distillation_loss")}


def stub_agent(cusrl, device="cpu"):
    """What a hook needs of an agent outside one; the actor is a real one with a 16-wide latent."""
    device = torch.device(device)
    actor = cusrl.Actor.Factory(cusrl.Mlp.Factory([32, 16], ends_with_activation=True), cusrl.NormalDist.Factory())(OBS, ACT)
    return SimpleNamespace(observation_dim=OBS, state_dim=STATE, action_dim=ACT, value_dim=VALUE, has_state=True, device=device,
                           setup_module=lambda m: m.to(device), actor=actor.to(device))


def _load(module, g, prefix, device):
    state = {str(name): torch.from_numpy(g[f"{prefix}param/{name}"]).to(device) for name in g[prefix + "param_names"]}
    module.load_state_dict(state)


def run_objective(cusrl, g, hook_kind, form, device="cpu"):
    """``(loss, {name: (gradient, golden gradient)}, golden loss)`` of one recorded stand-alone objective."""
    device = torch.device(device)

    def t(name):
        return torch.from_numpy(g[name]).to(device)

    agent = stub_agent(cusrl, device)
    prefix = f"obj_{hook_kind}_{form}_" if form is not None else f"obj_{hook_kind}_"
    if hook_kind == "distillation":
        hook = cusrl.hook.PolicyDistillationLoss(weight=1.5)
        hook.pre_init(agent)
        hook.init()
        mean = t("obj_distillation_mean").requires_grad_()
        loss = hook.objective({}, {"curr_action_dist": {"mean": mean}, "expert_action": t("obj_expert_action")})["distillation_loss"]
        loss.backward()
        return loss, {"d_mean": (mean.grad, g["obj_distillation_d_mean"])}, g["obj_distillation_loss"]
    batch = {name: t("obj_" + name) for name in ("observation", "state", "next_state", "action", "return", "value", "done")}
    if hook_kind == "estimation":
        hook = cusrl.hook.StateEstimation(cusrl.Mlp.Factory([12]), source_indices=slice(2, 14), target_indices=INDEX_FORMS[form],
                                          weight=0.7)
        key, module_name, latent = "state_estimation_loss", "estimator", None
    else:
        if hook_kind == "state_prediction":
            hook, key = cusrl.hook.StatePrediction(INDEX_FORMS[form], weight=0.3), "state_prediction_loss"
        elif hook_kind == "next_state_prediction":
            hook, key = cusrl.hook.NextStatePrediction(INDEX_FORMS[form], weight=0.2), "next_state_prediction_loss"
        else:
            hook = cusrl.hook.ReturnPrediction(weight=0.05, predicts_value_instead_of_return=form == "value")
            key = "return_prediction_loss"
        module_name, latent = "predictor", t(prefix + "latent").requires_grad_()
    hook.pre_init(agent)
    hook.init()
    module = getattr(hook, module_name)
    _load(module, g, prefix, device)
    if latent is not None:
        agent.actor.intermediate_repr["backbone.output"] = latent
    loss = hook.objective({}, batch)[key]
    loss.backward()
    grads = {"grad": (torch.cat([p.grad.reshape(-1) for p in module.parameters()]), g[prefix + "grad"])}
    if latent is not None:
        grads["d_latent"] = (latent.grad, g[prefix + "d_latent"])
    return loss, grads, g[prefix + "loss"]


def privileged_hooks(cusrl, tag):
    """The composition of update trace ``tag`` (make_privileged_golden.privileged_hooks), behind ``entropy_loss``."""
    if tag == "pa":
        hooks = [cusrl.hook.StateEstimation(cusrl.Mlp.Factory([12]), weight=0.5)]
    elif tag == "pb":
        hooks = [cusrl.hook.StatePrediction([5, 0, 5, 2], weight=0.1), cusrl.hook.ReturnPrediction(weight=0.05)]
    else:
        class ExpertAction(cusrl.Hook):
            rollout_capture_safe = True

            def post_step(self, transition):
                transition["expert_action"] = torch.tanh(transition["observation"][..., :ACT])

        hooks = [ExpertAction(), cusrl.hook.NextStatePrediction(slice(1, None, 2), weight=0.1),
                 cusrl.hook.PolicyDistillationLoss(weight=0.25)]
    placed, after = [], "entropy_loss"
    for hook in hooks:
        placed.append((hook, {"after": after}))
        after = hook.name
    return placed


def column_mse_f64(prediction, target, columns, weight):
    """The formula of include/cusrl_hip.h in float64 on the host: ``(loss, d loss / d prediction)``."""
    p = prediction.detach().cpu().numpy().astype(np.float64)
    t = target.detach().cpu().numpy().astype(np.float64)
    t = t[..., :p.shape[-1]] if columns is None else t[..., np.asarray(columns)]
    diff = p - t
    return weight * np.mean(diff * diff), 2.0 * weight / diff.size * diff
