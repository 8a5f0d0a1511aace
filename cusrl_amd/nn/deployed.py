"""A trained actor as a self-contained policy: what ``ActorCritic.export`` writes and what a robot or an evaluation loop runs
(counterpart of the reference's exported module — cusrl/template/actor_critic.py:332-418, cusrl/nn/layer/export.py — without
graph tracing, ONNX or TorchScript).

The file (``torch.save`` of ``{"spec": {...}, "tensors": {...}}``, format ``"cusrl_amd.policy"``, version 1) holds plain Python
values and CPU tensors only and is only ever read with ``weights_only=True``: nothing in it is executed.  Its spec is an ordered
list of stages out of a closed set::

    [nan_to_num] [normalize] (mlp | rnn)* head [action_affine] [action_clip]

``nan_to_num``: the replacement values of ``ObservationNanToNum``; ``normalize``: mean, std, clamp and epsilon, as
``RunningMeanStd.normalize``; ``mlp``: ``Linear`` + activation layers sharing one activation out of ReLU, ELU(alpha) and Tanh
(``ExpertPolicy``'s rules); ``rnn``: a GRU, LSTM or vanilla RNN core (the ``nn.RNNBase`` parameters) with its ``output_proj``;
``head``: the distribution's ``mean_head``; ``action_affine``: ``action * scale + shift``; ``action_clip``: ``clip(action, lo, hi)``.

``policy(observation [B, K]) -> action [B, A]`` is deterministic (the mean of a Normal distribution) and runs without a gradient.
A recurrent policy keeps its memory ``[B, memory_dim]`` — per ``rnn`` stage the hidden state ``[layers * hidden]`` and, for an
LSTM, the cell state behind it — allocates it at the first call and updates it in place; ``reset(done)`` zeroes rows.

On an MI355X a contiguous fp32 ``[B, K]`` input outside autocast costs one ``cusrl_deploy_prologue`` launch for everything in
front of the first GEMM, the existing launches per ``mlp`` / ``rnn`` stage (bias-free ``torch.mm`` + ``cusrl_bias_act``, or
``cusrl_mlp2_forward`` for the shape it takes; the step kernels of nn/gru.py) and one ``cusrl_deploy_epilogue`` launch behind the
head's bias-free GEMM, which also zeroes the memory rows of ``done`` when the caller passes it ("Deployment").  Any
other input evaluates the torch expression in fp32; on the CPU that is a host form (``utils.misc.host_form``)."""

from __future__ import annotations

import os
from collections.abc import Mapping, Sequence

import torch
from torch import Tensor, nn
from torch.nn import functional as F

__all__ = ["DeployedPolicy"]

FORMAT = "cusrl_amd.policy"
VERSION = 1
STAGE_KINDS = ("nan_to_num", "normalize", "mlp", "rnn", "head", "action_affine", "action_clip")
_ACTIVATIONS = ("ReLU", "ELU", "Tanh")
_RNN_TYPES = ("GRU", "LSTM", "RNN")


def _frozen(tensor: Tensor) -> Tensor:
    return tensor.detach().to(dtype=torch.float32).clone().contiguous()


def _vector(tensors: Mapping[str, Tensor], name: str, width: int, kind: str) -> Tensor:
    tensor = tensors.get(name)
    if not isinstance(tensor, Tensor) or tuple(tensor.shape) != (width,):
        found = "nothing" if tensor is None else f"shape {tuple(tensor.shape)}" if isinstance(tensor, Tensor) else type(tensor).__name__
        raise ValueError(f"Stage '{kind}': '{name}' must be a tensor of shape ({width},); found {found}")
    return tensor


class DeployedPolicy(nn.Module):
    """``stages``: a sequence of ``(meta, tensors)`` — ``meta`` a dict of plain values with ``"kind"`` out of
    :data:`STAGE_KINDS`, ``tensors`` the stage's tensors by name (see :meth:`ActorCritic.export`, the one writer).  Every tensor
    is copied into a detached fp32 buffer (an ``rnn`` stage's into a frozen ``nn.RNNBase``)."""

    def __init__(self, stages: Sequence[tuple[Mapping, Mapping[str, Tensor]]], observation_dim: int, action_dim: int):
        super().__init__()
        self.observation_dim, self.action_dim = int(observation_dim), int(action_dim)
        self._stages: list[dict] = []
        self._memory: Tensor | None = None
        order = {kind: rank for rank, kind in enumerate(("nan_to_num", "normalize", "body", "head", "action_affine", "action_clip"))}
        width, rank, offset = self.observation_dim, -1, 0
        for index, (meta, tensors) in enumerate(stages):
            meta, kind = dict(meta), meta.get("kind")
            if kind not in STAGE_KINDS:
                raise ValueError(f"Unknown stage kind {kind!r}; expected one of {list(STAGE_KINDS)}")
            this = order["body" if kind in ("mlp", "rnn") else kind]
            if this < rank or (this == rank and kind not in ("mlp", "rnn")):
                raise ValueError(f"Stage {index} ('{kind}') is out of order: a policy is [nan_to_num] [normalize] (mlp | rnn)* head "
                                 "[action_affine] [action_clip]")
            rank = this
            width, offset = getattr(self, "_add_" + kind)(index, meta, tensors, width, offset)
            self._stages.append(meta)
        if not any(meta["kind"] == "head" for meta in self._stages):
            raise ValueError("A policy needs a 'head' stage")
        if width != self.action_dim:
            raise ValueError(f"The stages end with width {width}, not with action_dim = {self.action_dim}")
        self.memory_dim = offset
        self.is_recurrent = offset > 0

    # ---- stages
    def _buffer(self, index: int, name: str, tensor: Tensor) -> None:
        self.register_buffer(f"s{index}_{name}", _frozen(tensor))

    def _get(self, index: int, name: str) -> Tensor:
        return getattr(self, f"s{index}_{name}")

    def _add_nan_to_num(self, index, meta, tensors, width, offset):
        for name in ("nan", "posinf", "neginf"):
            meta[name] = float(meta.get(name, 0.0))
        return width, offset

    def _add_normalize(self, index, meta, tensors, width, offset):
        clamp = meta.get("clamp")
        if clamp is not None and not clamp > 0:
            raise ValueError("Stage 'normalize': 'clamp' must be None or a positive value")
        meta["clamp"], meta["epsilon"] = (None if clamp is None else float(clamp)), float(meta.get("epsilon", 1e-8))
        for name in ("mean", "std"):
            self._buffer(index, name, _vector(tensors, name, width, "normalize"))
        return width, offset

    def _add_mlp(self, index, meta, tensors, width, offset):
        if meta.get("activation") not in _ACTIVATIONS:
            raise ValueError(f"Stage 'mlp': unsupported activation {meta.get('activation')!r}; expected one of {list(_ACTIVATIONS)}")
        meta["alpha"], meta["num_layers"] = float(meta.get("alpha", 1.0)), int(meta["num_layers"])
        if meta["num_layers"] < 1:
            raise ValueError("Stage 'mlp': needs at least one layer")
        for layer in range(meta["num_layers"]):
            weight = tensors.get(f"weight_{layer}")
            if not isinstance(weight, Tensor) or weight.dim() != 2 or weight.shape[1] != width:
                raise ValueError(f"Stage 'mlp': 'weight_{layer}' does not continue a stack of width {width}")
            self._buffer(index, f"weight_{layer}", weight)
            self._buffer(index, f"bias_{layer}", _vector(tensors, f"bias_{layer}", weight.shape[0], "mlp"))
            width = weight.shape[0]
        return width, offset

    def _add_rnn(self, index, meta, tensors, width, offset):
        from cusrl_amd.nn.rnn import _Gru, _Lstm, _VanillaRnn

        kind = meta.get("type")
        if kind not in _RNN_TYPES:
            raise ValueError(f"Stage 'rnn': unsupported type {kind!r}; expected one of {list(_RNN_TYPES)}")
        layers, hidden, bias = int(meta["num_layers"]), int(meta["hidden_size"]), bool(meta.get("bias", True))
        meta.update(num_layers=layers, hidden_size=hidden, bias=bias, output_proj=bool(meta.get("output_proj", False)))
        common = dict(input_size=width, hidden_size=hidden, num_layers=layers, bias=bias)
        if kind == "GRU":
            core = _Gru(**common)
        elif kind == "LSTM":
            core = _Lstm(**common)
        else:
            meta["nonlinearity"] = str(meta.get("nonlinearity", "tanh"))
            core = _VanillaRnn(nonlinearity=meta["nonlinearity"], **common)
        for name, parameter in core.named_parameters():
            given = tensors.get(name)
            if not isinstance(given, Tensor) or given.shape != parameter.shape:
                found = "nothing" if given is None else f"shape {tuple(given.shape)}"
                raise ValueError(f"Stage 'rnn': '{name}' must have shape {tuple(parameter.shape)}; found {found}")
            parameter.data = _frozen(given)
            parameter.requires_grad_(False)
        self.add_module(f"s{index}_core", core.eval())
        width = hidden
        if meta["output_proj"]:
            weight = tensors.get("proj_weight")
            if not isinstance(weight, Tensor) or weight.dim() != 2 or weight.shape[1] != hidden:
                raise ValueError(f"Stage 'rnn': 'proj_weight' does not project a hidden state of width {hidden}")
            self._buffer(index, "proj_weight", weight)
            self._buffer(index, "proj_bias", _vector(tensors, "proj_bias", weight.shape[0], "rnn"))
            width = weight.shape[0]
        meta["memory_offset"] = offset
        return width, offset + layers * hidden * (2 if kind == "LSTM" else 1)

    def _add_head(self, index, meta, tensors, width, offset):
        weight = tensors.get("weight")
        if not isinstance(weight, Tensor) or weight.dim() != 2 or weight.shape[1] != width:
            raise ValueError(f"Stage 'head': 'weight' does not continue a stack of width {width}")
        self._buffer(index, "weight", weight)
        self._buffer(index, "bias", _vector(tensors, "bias", weight.shape[0], "head"))
        return weight.shape[0], offset

    def _add_action_affine(self, index, meta, tensors, width, offset):
        for name in ("scale", "shift"):
            self._buffer(index, name, _vector(tensors, name, width, "action_affine"))
        return width, offset

    def _add_action_clip(self, index, meta, tensors, width, offset):
        for name in ("lo", "hi"):
            self._buffer(index, name, _vector(tensors, name, width, "action_clip"))
        return width, offset

    def _stage(self, kind: str):
        """``(index, meta)`` of the one stage of a kind outside the body, or ``(None, None)``."""
        for index, meta in enumerate(self._stages):
            if meta["kind"] == kind:
                return index, meta
        return None, None

    # ---- file format
    def spec(self) -> dict:
        stages = [{key: value for key, value in meta.items() if key != "memory_offset"} for meta in self._stages]
        return {"format": FORMAT, "version": VERSION, "stages": stages, "observation_dim": self.observation_dim,
                "action_dim": self.action_dim, "is_recurrent": self.is_recurrent, "memory_dim": self.memory_dim}

    def tensors(self) -> dict[str, Tensor]:
        """Every tensor of the policy as ``"<stage index>.<name>"``, the way the file keeps them."""
        found = {}
        for index, meta in enumerate(self._stages):
            prefix = f"s{index}_"
            for name, buffer in self.named_buffers(recurse=False):
                if name.startswith(prefix):
                    found[f"{index}.{name[len(prefix):]}"] = buffer
            if meta["kind"] == "rnn":
                for name, parameter in getattr(self, prefix + "core").named_parameters():
                    found[f"{index}.{name}"] = parameter.data
        return found

    def save(self, path) -> None:
        """``torch.save`` of ``{"spec": {...}, "tensors": {...}}``: plain Python values and CPU tensors only, so the file loads
        with ``weights_only=True``."""
        tensors = {name: tensor.detach().cpu().clone() for name, tensor in self.tensors().items()}
        torch.save({"spec": self.spec(), "tensors": tensors}, os.fspath(path))

    @classmethod
    def load(cls, path, map_location=None) -> "DeployedPolicy":
        policy = cls.try_load(path, map_location)
        if policy is None:
            raise ValueError(f"'{os.fspath(path)}' is not a file in the '{FORMAT}' format")
        return policy

    @classmethod
    def try_load(cls, path, map_location=None) -> "DeployedPolicy | None":
        """The policy stored in ``path``, or None when the file is something else (an ``ExpertPolicy`` file, a TorchScript
        archive, a checkpoint, garbage).  The file is only ever read with ``weights_only=True``: nothing in it is executed."""
        import zipfile

        if zipfile.is_zipfile(os.fspath(path)):
            with zipfile.ZipFile(os.fspath(path)) as archive:
                if any(name.endswith("/constants.pkl") for name in archive.namelist()):
                    return None  # a TorchScript archive (torch.load would hand it to torch.jit.load itself)
        try:
            data = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
        except FileNotFoundError:
            raise
        except Exception:  # not a weights-only archive
            return None
        spec = data.get("spec") if isinstance(data, dict) else None
        if not isinstance(spec, dict) or spec.get("format") != FORMAT:
            return None
        if spec.get("version") != VERSION:
            raise ValueError(f"'{os.fspath(path)}': unsupported '{FORMAT}' version {spec.get('version')!r} (this build reads {VERSION})")
        tensors = data["tensors"]
        stages = []
        for index, meta in enumerate(spec["stages"]):
            prefix = f"{index}."
            stages.append((meta, {name[len(prefix):]: tensor for name, tensor in tensors.items() if name.startswith(prefix)}))
        policy = cls(stages, spec["observation_dim"], spec["action_dim"])
        if policy.memory_dim != spec.get("memory_dim") or policy.is_recurrent != spec.get("is_recurrent"):
            raise ValueError(f"'{os.fspath(path)}': the stages keep a memory of {policy.memory_dim} values per row, the spec says "
                             f"{spec.get('memory_dim')!r}")
        return policy if map_location is None else policy.to(map_location)

    # ---- memory
    @property
    def memory(self) -> Tensor | None:
        """``[B, memory_dim]`` (None before the first call and for a feed-forward policy); assignable."""
        return self._memory

    @memory.setter
    def memory(self, value: Tensor | None) -> None:
        if value is None:
            self._memory = None
            return
        if not self.is_recurrent:
            raise ValueError("A feed-forward policy keeps no memory")
        if not isinstance(value, Tensor) or value.dim() != 2 or value.shape[1] != self.memory_dim:
            raise ValueError(f"'memory' must be a [B, {self.memory_dim}] tensor")
        self._memory = value.detach().to(dtype=torch.float32).clone().contiguous()

    def reset(self, done: Tensor | None = None) -> None:
        """Zero the memory rows where ``done`` (``[B]`` or ``[B, 1]``, bool) is set; every row when ``done`` is None."""
        if self._memory is None:
            return
        if done is None:
            self._memory.zero_()
            return
        done = self._done(done, self._memory.shape[0], self._memory.device)
        self._memory[done] = 0

    @staticmethod
    def _done(done, rows: int, device) -> Tensor:
        done = torch.as_tensor(done, device=device)
        if done.dtype != torch.bool:
            raise TypeError(f"'done' must have dtype bool, got {done.dtype}")
        if done.dim() == 2 and done.shape[1] == 1:
            done = done.squeeze(-1)
        if tuple(done.shape) != (rows,):
            raise ValueError(f"'done' must have shape ({rows},) or ({rows}, 1); got {tuple(done.shape)}")
        return done.contiguous()

    def _ensure_memory(self, rows: int, device) -> Tensor | None:
        if not self.is_recurrent:
            return None
        if self._memory is None:
            self._memory = torch.zeros(rows, self.memory_dim, dtype=torch.float32, device=device)
        elif self._memory.shape[0] != rows:
            raise ValueError(f"The policy's memory holds {self._memory.shape[0]} rows, the observation {rows}; assign "
                             "'memory = None' to start over with another batch size")
        elif self._memory.device != device:
            self._memory = self._memory.to(device)
        return self._memory

    def _apply(self, fn, *args, **kwargs):
        result = super()._apply(fn, *args, **kwargs)
        if self._memory is not None:
            self._memory = fn(self._memory)
        return result

    # ---- evaluation
    def _native(self, observation) -> bool:
        head = self._get(self._stage("head")[0], "weight")
        return (isinstance(observation, Tensor) and observation.is_cuda and observation.dim() == 2 and observation.numel() > 0
                and observation.dtype == torch.float32 and observation.is_contiguous()
                and observation.shape[1] == self.observation_dim and head.device == observation.device
                and not torch.is_autocast_enabled("cuda"))

    @torch.no_grad()
    def forward(self, observation: Tensor, done: Tensor | None = None) -> Tensor:
        """The action for ``observation [B, K]``.  ``done`` (``[B]`` or ``[B, 1]`` bool): the envs that finished WITH this step —
        their memory rows are zeroed behind it, as a ``reset(done)`` after the call would."""
        if not isinstance(observation, Tensor) or observation.dim() != 2 or observation.shape[1] != self.observation_dim:
            found = tuple(observation.shape) if isinstance(observation, Tensor) else type(observation).__name__
            raise ValueError(f"'observation' must be a [B, {self.observation_dim}] tensor; got {found}")
        memory = self._ensure_memory(observation.shape[0], observation.device)
        if done is not None:
            done = self._done(done, observation.shape[0], observation.device)
        if self._native(observation):
            return self._forward_native(observation, memory, done)
        if not observation.is_cuda:
            from cusrl_amd.utils.misc import host_form

            host_form("DeployedPolicy")
        # the torch expression, in fp32 whatever autocast says
        with torch.autocast(device_type=observation.device.type, enabled=False):
            action = self._forward_torch(observation.float(), memory)
        if done is not None and memory is not None:
            memory[done] = 0
        return action

    def _step_rnn(self, index: int, meta: dict, x: Tensor, memory: Tensor) -> Tensor:
        """One step of an ``rnn`` stage: its columns of ``memory`` in, the new state written back in place."""
        core = getattr(self, f"s{index}_core")
        size, lo = meta["num_layers"] * meta["hidden_size"], meta["memory_offset"]
        hidden = memory[:, lo:lo + size]
        if meta["type"] == "LSTM":
            cell = memory[:, lo + size:lo + 2 * size]
            latent, state = core(x.unsqueeze(0), {"hidden": hidden, "cell": cell})
            hidden.copy_(state["hidden"])
            cell.copy_(state["cell"])
        else:
            latent, state = core(x.unsqueeze(0), hidden)
            hidden.copy_(state)
        return latent.squeeze(0)

    def _forward_torch(self, x: Tensor, memory: Tensor | None) -> Tensor:
        for index, meta in enumerate(self._stages):
            kind = meta["kind"]
            if kind == "nan_to_num":
                x = x.nan_to_num(nan=meta["nan"], posinf=meta["posinf"], neginf=meta["neginf"])
            elif kind == "normalize":
                x = (x - self._get(index, "mean")) / self._get(index, "std")
                if meta["clamp"] is not None:
                    x = x.clamp(-meta["clamp"], meta["clamp"])
            elif kind == "mlp":
                for layer in range(meta["num_layers"]):
                    x = F.linear(x, self._get(index, f"weight_{layer}"), self._get(index, f"bias_{layer}"))
                    x = (F.elu(x, meta["alpha"]) if meta["activation"] == "ELU" else torch.relu(x) if meta["activation"] == "ReLU"
                         else torch.tanh(x))
            elif kind == "rnn":
                x = self._step_rnn(index, meta, x, memory)
                if meta["output_proj"]:
                    x = F.linear(x, self._get(index, "proj_weight"), self._get(index, "proj_bias"))
            elif kind == "head":
                x = F.linear(x, self._get(index, "weight"), self._get(index, "bias"))
            elif kind == "action_affine":
                x = x * self._get(index, "scale") + self._get(index, "shift")
            else:
                x = torch.clamp(x, self._get(index, "lo"), self._get(index, "hi"))
        return x

    def _forward_native(self, x: Tensor, memory: Tensor | None, done: Tensor | None) -> Tensor:
        from cusrl_amd import ops

        sanitise, normalise = self._stage("nan_to_num"), self._stage("normalize")
        if sanitise[0] is not None or normalise[0] is not None:  # everything in front of the first GEMM: ONE launch
            replace = None if sanitise[0] is None else (sanitise[1]["nan"], sanitise[1]["posinf"], sanitise[1]["neginf"])
            mean = std = clamp = None
            if normalise[0] is not None:
                mean, std, clamp = self._get(normalise[0], "mean"), self._get(normalise[0], "std"), normalise[1]["clamp"]
            x = ops.deploy_prologue(x, replace, mean, std, clamp)
        head_index, _ = self._stage("head")
        affine, clip = self._stage("action_affine")[0], self._stage("action_clip")[0]
        tail = affine is not None or clip is not None or (done is not None and memory is not None)
        body = [(index, meta) for index, meta in enumerate(self._stages) if meta["kind"] in ("mlp", "rnn")]
        head_weight, head_bias = self._get(head_index, "weight"), self._get(head_index, "bias")
        y = None
        if len(body) == 1 and body[0][1]["kind"] == "mlp" and body[0][1]["activation"] == "ReLU" and body[0][1]["num_layers"] == 2:
            # Linear / ReLU / Linear / ReLU in front of the head: the one-launch inference pass, where it takes the shape —
            # without the head's bias when the epilogue follows (which then adds it)
            index = body[0][0]
            layers = (self._get(index, "weight_0"), self._get(index, "bias_0"), self._get(index, "weight_1"), self._get(index, "bias_1"),
                      head_weight, None if tail else head_bias)
            if ops.mlp2_forward_supported(x, layers):
                y = ops.mlp2_forward(x, layers)
                if not tail:
                    return y
        if y is None:
            for index, meta in body:
                if meta["kind"] == "mlp":
                    for layer in range(meta["num_layers"]):
                        x = torch.mm(x, self._get(index, f"weight_{layer}").t())  # bias-free library GEMM + ONE launch behind it
                        ops.bias_act(x, self._get(index, f"bias_{layer}"), meta["activation"], meta["alpha"], out=x)
                else:
                    x = self._step_rnn(index, meta, x, memory)
                    if meta["output_proj"]:
                        x = torch.mm(x.contiguous(), self._get(index, "proj_weight").t())
                        ops.bias_act(x, self._get(index, "proj_bias"), "identity", out=x)
            y = torch.mm(x.contiguous(), head_weight.t())
        # everything behind the last GEMM, the memory rows of `done` included: ONE launch
        ops.deploy_epilogue_(y, head_bias,
                             None if affine is None else self._get(affine, "scale"), None if affine is None else self._get(affine, "shift"),
                             None if clip is None else self._get(clip, "lo"), None if clip is None else self._get(clip, "hi"),
                             done if memory is not None else None, memory)
        return y

    def extra_repr(self) -> str:
        kinds = [meta["type"] if meta["kind"] == "rnn" else meta["kind"] for meta in self._stages]
        return (f"observation_dim={self.observation_dim}, action_dim={self.action_dim}, stages={kinds}, "
                f"memory_dim={self.memory_dim}")
