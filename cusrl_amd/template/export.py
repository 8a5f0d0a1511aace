"""What ``ActorCritic.export`` writes: the agent's actor, with the observation stages its hooks contribute, as the stage list
of a ``nn.DeployedPolicy`` (cusrl_amd/nn/deployed.py; counterpart of cusrl/template/actor_critic.py:332-418 without graph
tracing).  An agent the stage set cannot express is refused with a ``ValueError`` naming what was found: a file that silently
differs from the agent is worse than no file."""

from __future__ import annotations

import os

import torch
from torch import nn

from cusrl_amd.template.hook import Hook

__all__ = ["actor_stages", "export_policy", "hook_stages"]

_ACTIVATIONS = {"ReLU": nn.ReLU, "ELU": nn.ELU, "Tanh": nn.Tanh}
_WHO = "ActorCritic.export"


def _name(module) -> str:
    return repr(module) if isinstance(module, nn.Module) else type(module).__name__


def _mlp_stage(mlp) -> tuple[dict, dict]:
    """``ExpertPolicy.from_actor``'s rules: ``Linear`` (with a bias) + activation pairs, one activation out of ReLU, ELU and
    Tanh, no Dropout, an activation behind the last layer."""
    layers = list(mlp.layers)
    tensors, activations = {}, []
    position = 0
    while position < len(layers):
        linear = layers[position]
        if not isinstance(linear, nn.Linear) or linear.bias is None:
            raise ValueError(f"{_WHO}: layer {position} of the Mlp is {_name(linear)} where a Linear with a bias was expected")
        if position + 1 >= len(layers):
            raise ValueError(f"{_WHO}: the Mlp ends with a Linear that has no activation behind it (ends_with_activation=False); "
                             "every layer of an 'mlp' stage needs the shared activation")
        activation = layers[position + 1]
        if isinstance(activation, nn.Dropout) or (position + 2 < len(layers) and isinstance(layers[position + 2], nn.Dropout)):
            raise ValueError(f"{_WHO}: the Mlp holds Dropout layers; an exported policy needs dropout=0")
        if type(activation) not in _ACTIVATIONS.values():
            raise ValueError(f"{_WHO}: layer {position + 1} of the Mlp is {_name(activation)}; the activation must be one of "
                             f"{sorted(_ACTIVATIONS)}")
        tensors[f"weight_{len(activations)}"], tensors[f"bias_{len(activations)}"] = linear.weight, linear.bias
        activations.append(activation)
        position += 2
    kinds = {(type(a).__name__, float(getattr(a, "alpha", 1.0))) for a in activations}
    if len(kinds) > 1:
        raise ValueError(f"{_WHO}: the layers of an Mlp must share one activation; found mixed activations "
                         + ", ".join(_name(a) for a in activations))
    if not kinds:
        raise ValueError(f"{_WHO}: the Mlp has no layer")
    (activation_name, alpha), = kinds
    return {"kind": "mlp", "activation": activation_name, "alpha": alpha, "num_layers": len(activations)}, tensors


def _rnn_stage(rnn) -> tuple[dict, dict]:
    core = rnn.rnn
    kind = "GRU" if isinstance(core, nn.GRU) else "LSTM" if isinstance(core, nn.LSTM) else "RNN" if isinstance(core, nn.RNN) else None
    if kind is None:
        raise ValueError(f"{_WHO}: the recurrent core is {type(core).__name__}; an 'rnn' stage is a GRU, an LSTM or a vanilla RNN")
    if core.bidirectional or core.batch_first or getattr(core, "proj_size", 0) or (core.dropout and core.num_layers > 1):
        raise ValueError(f"{_WHO}: the {kind} core is bidirectional, batch-first, projected or has Dropout between its layers "
                         f"({core}); an 'rnn' stage is a plain time-major core")
    meta = {"kind": "rnn", "type": kind, "num_layers": core.num_layers, "hidden_size": core.hidden_size, "bias": bool(core.bias)}
    if kind == "RNN":
        meta["nonlinearity"] = core.nonlinearity
    tensors = dict(core.named_parameters())
    proj = rnn.output_proj
    meta["output_proj"] = isinstance(proj, nn.Linear)
    if isinstance(proj, nn.Linear):
        if proj.bias is None:
            raise ValueError(f"{_WHO}: the 'output_proj' of the {kind} backbone has no bias")
        tensors["proj_weight"], tensors["proj_bias"] = proj.weight, proj.bias
    elif not isinstance(proj, nn.Identity):
        raise ValueError(f"{_WHO}: the 'output_proj' of the {kind} backbone is {_name(proj)}; a Linear or nothing was expected")
    return meta, tensors


def _backbone_stages(backbone) -> list[tuple[dict, dict]]:
    from cusrl_amd.nn.module import Mlp
    from cusrl_amd.nn.rnn import Rnn
    from cusrl_amd.nn.sequential import Sequential

    if type(backbone) is Mlp:
        return [_mlp_stage(backbone)]
    if isinstance(backbone, Rnn):
        return [_rnn_stage(backbone)]
    if type(backbone) is Sequential:
        return [stage for layer in backbone.layers for stage in _backbone_stages(layer)]
    kind = "recurrent " if getattr(backbone, "is_recurrent", False) else ""
    raise ValueError(f"{_WHO}: the stage set expresses Mlp and Rnn (GRU, LSTM, vanilla) backbones and a Sequential of them; found "
                     f"the {kind}backbone {type(backbone).__name__}")


def actor_stages(actor) -> list[tuple[dict, dict]]:
    """The ``mlp`` / ``rnn`` stages of ``actor``'s backbone and the ``head`` stage of its distribution's ``mean_head`` — the
    deterministic action of a Normal distribution is its mean."""
    from cusrl_amd.nn.actor import Actor
    from cusrl_amd.nn.distribution import _Normal

    if type(actor) is not Actor:
        raise ValueError(f"{_WHO}: the actor is a {type(actor).__name__}; only a plain Actor (a backbone in front of a distribution) "
                         "can be exported")
    distribution = actor.distribution
    head = getattr(distribution, "mean_head", None)
    if not isinstance(distribution, _Normal):
        raise ValueError(f"{_WHO}: the distribution is {type(distribution).__name__}; only a Normal distribution, whose "
                         "deterministic action is the output of its linear 'mean_head', can be exported")
    if not isinstance(head, nn.Linear) or head.bias is None:
        raise ValueError(f"{_WHO}: the distribution's 'mean_head' is {_name(head)} where a Linear with a bias was expected")
    if actor.backbone_kwargs or actor.distribution_kwargs:
        raise ValueError(f"{_WHO}: the actor carries 'backbone_kwargs' / 'distribution_kwargs' "
                         f"({actor.backbone_kwargs}, {actor.distribution_kwargs}); a stage list has no place for them")
    return [*_backbone_stages(actor.backbone), ({"kind": "head"}, {"weight": head.weight, "bias": head.bias})]


def hook_stages(hooks, which: str = "actor") -> list[tuple[dict, dict]]:
    """What the hooks that act at deployment (active, not training-only) contribute, in hook order.  A hook that overrides
    ``pre_act`` — the place where observations are rewritten — without overriding ``export_stages`` is refused."""
    stages = []
    for hook in hooks:
        if not hook.active or hook.training_only:
            continue
        if type(hook).pre_act is not Hook.pre_act and type(hook).export_stages is Hook.export_stages:
            raise ValueError(f"{_WHO}: hook '{hook.name}' ({type(hook).__name__}) overrides 'pre_act', where observations are "
                             "rewritten, but contributes no export stage; the file would differ from the agent.  A hook whose "
                             "'pre_act' leaves the actor's observation alone says so by overriding 'export_stages' to return ()")
        stages.extend(hook.export_stages(which))
    return stages


def _action_vector(value, width: int, name: str) -> torch.Tensor:
    tensor = torch.as_tensor(value, dtype=torch.float32).detach().cpu()
    if tensor.dim() == 0:
        tensor = tensor.expand(width)
    if tuple(tensor.shape) != (width,):
        raise ValueError(f"{_WHO}: '{name}' must be a scalar or have shape ({width},); got {tuple(tensor.shape)}")
    return tensor.contiguous()


def export_policy(agent, output_dir, name: str = "policy", *, with_environment_normalization: bool = True, action_clip=None):
    """Build the ``DeployedPolicy`` of ``agent`` and save it as ``<output_dir>/<name>.pt``; returns the path."""
    from cusrl_amd.nn.deployed import DeployedPolicy

    spec = agent.environment_spec
    stages = hook_stages(agent.hook) + actor_stages(agent.actor)
    if with_environment_normalization:
        if spec.get("observation_normalization") is not None:
            raise ValueError(f"{_WHO}: the environment spec carries 'observation_normalization', which has no place in front of the "
                             "hooks' stages; export with with_environment_normalization=False and normalise at the caller")
        denormalization = spec.get("action_denormalization")
        if denormalization is not None:
            scale, shift = denormalization
            stages.append(({"kind": "action_affine"}, {"scale": _action_vector(scale, agent.action_dim, "action_denormalization[0]"),
                                                       "shift": _action_vector(shift, agent.action_dim, "action_denormalization[1]")}))
    if action_clip is not None:
        lo, hi = action_clip
        stages.append(({"kind": "action_clip"}, {"lo": _action_vector(lo, agent.action_dim, "action_clip[0]"),
                                                 "hi": _action_vector(hi, agent.action_dim, "action_clip[1]")}))
    try:
        policy = DeployedPolicy(stages, agent.observation_dim, agent.action_dim)
    except ValueError as error:
        raise ValueError(f"{_WHO}: {error}") from error
    os.makedirs(os.fspath(output_dir), exist_ok=True)
    path = os.path.join(os.fspath(output_dir), f"{name}.pt")
    policy.save(path)
    return path
