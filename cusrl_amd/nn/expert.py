"""A frozen feed-forward expert policy: the teacher that ``hook.PolicyDistillation`` queries at every env step.

The reference's expert is a TorchScript file written by its ``export``, which this package does not have; an ``ExpertPolicy`` is
what a user of this package makes of a trained ``Actor`` instead (:meth:`ExpertPolicy.from_actor`, :meth:`save`,
:meth:`load`).  It is an optional observation normaliser (``(x - mean) / std``, clamped: ``RunningMeanStd.normalize``, whose
excluded channels simply carry mean 0 and std ~1), a stack of ``Linear`` + activation layers that share one activation out of
ReLU, ELU and Tanh, and a linear head.  Calling it returns the mean action, deterministically and without a gradient.

On an MI355X a contiguous fp32 ``[B, K]`` input outside autocast costs one ``cusrl_rms_normalize`` launch (with a normaliser)
and, per layer, one bias-free ``torch.mm`` plus one ``cusrl_bias_act`` launch ("Distillation").  Any other input
evaluates the torch expression in fp32; on the CPU that is a host form (``utils.misc.host_form``)."""

from __future__ import annotations

import os
from collections.abc import Sequence

import torch
from torch import Tensor, nn
from torch.nn import functional as F

__all__ = ["ExpertPolicy"]

FORMAT = "cusrl_amd.expert"
VERSION = 1
_ACTIVATIONS = {"ReLU": nn.ReLU, "ELU": nn.ELU, "Tanh": nn.Tanh}


class ExpertPolicy(nn.Module):
    """``weights[i]`` is ``[out_i, in_i]`` and ``biases[i]`` ``[out_i]``, as ``nn.Linear`` keeps them; the last pair is the
    head.  ``activation``: ``"ReLU"``, ``"ELU"`` (with ``alpha``) or ``"Tanh"``, behind every layer but the head.  ``mean`` /
    ``std`` (both or neither): the observation normaliser, clamped to ``[-clamp, clamp]`` unless ``clamp`` is None;
    ``epsilon`` records what the statistics' ``std = sqrt(var + epsilon)`` was computed with.  Every tensor is copied into a
    detached fp32 buffer."""

    def __init__(self, weights: Sequence[Tensor], biases: Sequence[Tensor], activation: str = "ReLU", alpha: float = 1.0,
                 mean: Tensor | None = None, std: Tensor | None = None, clamp: float | None = None, epsilon: float = 1e-8):
        super().__init__()
        if activation not in _ACTIVATIONS:
            raise ValueError(f"Unsupported expert activation '{activation}'; expected one of {sorted(_ACTIVATIONS)}")
        if not weights or len(weights) != len(biases):
            raise ValueError(f"An expert needs one bias per weight and at least a head; got {len(weights)} weights and "
                             f"{len(biases)} biases")
        if (mean is None) != (std is None):
            raise ValueError("'mean' and 'std' must be given together")
        if clamp is not None and clamp <= 0:
            raise ValueError("'clamp' must be None or a positive value")
        self.activation, self.alpha, self.clamp, self.epsilon = activation, float(alpha), clamp, float(epsilon)
        self.num_layers = len(weights)
        fan_in = weights[0].shape[1]
        for i, (weight, bias) in enumerate(zip(weights, biases)):
            if weight.dim() != 2 or weight.shape[1] != fan_in or tuple(bias.shape) != (weight.shape[0],):
                raise ValueError(f"Layer {i}: weight {tuple(weight.shape)} and bias {tuple(bias.shape)} do not continue a stack "
                                 f"of width {fan_in}")
            self.register_buffer(f"weight_{i}", _frozen(weight))
            self.register_buffer(f"bias_{i}", _frozen(bias))
            fan_in = weight.shape[0]
        self.input_dim, self.output_dim = weights[0].shape[1], fan_in
        if mean is not None:
            if tuple(mean.shape) != (self.input_dim,) or tuple(std.shape) != (self.input_dim,):
                raise ValueError(f"'mean' and 'std' must have shape ({self.input_dim},); got {tuple(mean.shape)} and "
                                 f"{tuple(std.shape)}")
            mean, std = _frozen(mean), _frozen(std)
        self.register_buffer("mean", mean)
        self.register_buffer("std", std)

    # ---- construction from a trained actor
    @classmethod
    def from_actor(cls, actor, normalizer=None) -> "ExpertPolicy":
        """The frozen copy of a trained ``Actor``: a feed-forward ``Mlp`` backbone of ``Linear`` + activation layers (one
        activation out of ReLU, ELU and Tanh, ``dropout=0``, ``ends_with_activation=True``) in front of a distribution with a
        linear ``mean_head``.  ``normalizer``: the ``RunningMeanStd`` the actor's observations went through.  Anything else
        raises ``ValueError`` naming what was found."""
        from cusrl_amd.nn.module import Mlp
        from cusrl_amd.nn.rms import RunningMeanStd

        backbone = getattr(actor, "backbone", None)
        if type(backbone) is not Mlp:
            kind = "recurrent " if getattr(backbone, "is_recurrent", False) else ""
            raise ValueError(f"ExpertPolicy.from_actor needs a feed-forward Mlp backbone; found the {kind}backbone "
                             f"{type(backbone).__name__}")
        head = getattr(getattr(actor, "distribution", None), "mean_head", None)
        if not isinstance(head, nn.Linear) or head.bias is None:
            raise ValueError("ExpertPolicy.from_actor needs a distribution with a linear 'mean_head' (with a bias); found "
                             f"{type(getattr(actor, 'distribution', None)).__name__} with mean_head {type(head).__name__}")
        layers = list(backbone.layers)
        weights, biases, activations = [], [], []
        position = 0
        while position < len(layers):
            linear = layers[position]
            if not isinstance(linear, nn.Linear) or linear.bias is None:
                raise ValueError(f"ExpertPolicy.from_actor: layer {position} of the backbone is {_name(linear)} where a Linear "
                                 "with a bias was expected")
            if position + 1 >= len(layers):
                raise ValueError("ExpertPolicy.from_actor: the backbone ends with a Linear that has no activation behind it "
                                 "(ends_with_activation=False); every layer in front of the head needs the shared activation")
            activation = layers[position + 1]
            if isinstance(activation, nn.Dropout) or (position + 2 < len(layers) and isinstance(layers[position + 2], nn.Dropout)):
                raise ValueError("ExpertPolicy.from_actor: the backbone holds Dropout layers; a frozen expert needs dropout=0")
            if type(activation) not in _ACTIVATIONS.values():
                raise ValueError(f"ExpertPolicy.from_actor: layer {position + 1} of the backbone is {_name(activation)}; the "
                                 f"activation must be one of {sorted(_ACTIVATIONS)}")
            weights.append(linear.weight)
            biases.append(linear.bias)
            activations.append(activation)
            position += 2
        kinds = {(type(a).__name__, float(getattr(a, "alpha", 1.0))) for a in activations}
        if len(kinds) > 1:
            found = ", ".join(_name(a) for a in activations)
            raise ValueError(f"ExpertPolicy.from_actor: the hidden layers must share one activation; found mixed activations {found}")
        if not kinds:
            raise ValueError("ExpertPolicy.from_actor: the backbone has no layer")
        (activation_name, alpha), = kinds
        mean = std = clamp = None
        epsilon = 1e-8
        if normalizer is not None:
            if not isinstance(normalizer, RunningMeanStd):
                raise ValueError(f"ExpertPolicy.from_actor: 'normalizer' must be a RunningMeanStd; found {type(normalizer).__name__}")
            mean, std, clamp, epsilon = normalizer.mean, normalizer.std, normalizer.clamp, normalizer.epsilon
        return cls([*weights, head.weight], [*biases, head.bias], activation_name, alpha, mean, std, clamp, epsilon)

    # ---- file format
    def spec(self) -> dict:
        return {"format": FORMAT, "version": VERSION, "activation": self.activation, "alpha": self.alpha, "clamp": self.clamp,
                "epsilon": self.epsilon, "num_layers": self.num_layers, "normalized": self.mean is not None}

    def save(self, path) -> None:
        """``torch.save`` of ``{"spec": {...}, "tensors": {...}}``: plain Python values and CPU tensors only, so the file loads
        with ``weights_only=True``."""
        tensors = {name: buffer.detach().cpu().clone() for name, buffer in self.named_buffers()}
        torch.save({"spec": self.spec(), "tensors": tensors}, os.fspath(path))

    @classmethod
    def load(cls, path, map_location=None) -> "ExpertPolicy":
        expert = cls.try_load(path, map_location)
        if expert is None:
            raise ValueError(f"'{os.fspath(path)}' is not a file in the '{FORMAT}' format")
        return expert

    @classmethod
    def try_load(cls, path, map_location=None) -> "ExpertPolicy | None":
        """The expert stored in ``path``, or None when the file is something else (a TorchScript archive, say).  The file is
        only ever read with ``weights_only=True``: nothing in it is executed."""
        import zipfile

        if zipfile.is_zipfile(os.fspath(path)):
            with zipfile.ZipFile(os.fspath(path)) as archive:
                if any(name.endswith("/constants.pkl") for name in archive.namelist()):
                    return None  # a TorchScript archive (torch.load would hand it to torch.jit.load itself)
        try:
            data = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
        except FileNotFoundError:
            raise
        except Exception:  # not a weights-only archive: a TorchScript file, a pickle with code in it, another format
            return None
        spec = data.get("spec") if isinstance(data, dict) else None
        if not isinstance(spec, dict) or spec.get("format") != FORMAT:
            return None
        if spec.get("version") != VERSION:
            raise ValueError(f"'{os.fspath(path)}': unsupported '{FORMAT}' version {spec.get('version')!r} (this build reads {VERSION})")
        tensors = data["tensors"]
        count = int(spec["num_layers"])
        expert = cls([tensors[f"weight_{i}"] for i in range(count)], [tensors[f"bias_{i}"] for i in range(count)],
                     spec["activation"], spec["alpha"], tensors.get("mean") if spec.get("normalized") else None,
                     tensors.get("std") if spec.get("normalized") else None, spec["clamp"], spec["epsilon"])
        return expert if map_location is None else expert.to(map_location)

    # ---- evaluation
    def layers(self) -> list[tuple[Tensor, Tensor]]:
        return [(getattr(self, f"weight_{i}"), getattr(self, f"bias_{i}")) for i in range(self.num_layers)]

    def reset(self, done=None) -> None:
        """Nothing to reset (a feed-forward policy); ``PolicyDistillation`` calls it after every env step when present."""

    def _native(self, observation) -> bool:
        return (isinstance(observation, Tensor) and observation.is_cuda and observation.dim() == 2 and observation.numel() > 0
                and observation.dtype == torch.float32 and observation.is_contiguous() and observation.shape[1] == self.input_dim
                and self.weight_0.device == observation.device and not torch.is_autocast_enabled("cuda"))

    @torch.no_grad()
    def forward(self, observation: Tensor) -> Tensor:
        if self._native(observation):
            from cusrl_amd import ops

            x = observation
            if self.mean is not None:
                x = ops.rms_normalize(x, self.mean, self.std, self.clamp)
            last = self.num_layers - 1
            for i, (weight, bias) in enumerate(self.layers()):
                x = torch.mm(x, weight.t())  # bias-free library GEMM; bias and activation are the one launch behind it
                ops.bias_act(x, bias, "identity" if i == last else self.activation, self.alpha, out=x)
            return x
        if not observation.is_cuda:
            from cusrl_amd.utils.misc import host_form

            host_form("ExpertPolicy")
        # the torch expression, in fp32 whatever autocast says (a frozen teacher is not part of the mixed-precision region)
        with torch.autocast(device_type=observation.device.type, enabled=False):
            x = observation.float()
            if self.mean is not None:
                x = (x - self.mean) / self.std
                if self.clamp is not None:
                    x = x.clamp(-self.clamp, self.clamp)
            last = self.num_layers - 1
            for i, (weight, bias) in enumerate(self.layers()):
                x = F.linear(x, weight, bias)
                if i != last:
                    x = F.elu(x, self.alpha) if self.activation == "ELU" else torch.relu(x) if self.activation == "ReLU" else torch.tanh(x)
            return x

    def extra_repr(self) -> str:
        widths = [self.input_dim, *(weight.shape[0] for weight, _ in self.layers())]
        return (f"widths={widths}, activation={self.activation}, alpha={self.alpha}, normalized={self.mean is not None}, "
                f"clamp={self.clamp}")


def _frozen(tensor: Tensor) -> Tensor:
    return tensor.detach().to(dtype=torch.float32).clone().contiguous()


def _name(module) -> str:
    return repr(module) if isinstance(module, nn.Module) else type(module).__name__
