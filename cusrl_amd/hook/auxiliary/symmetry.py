"""Mirror symmetry (counterpart of cusrl/hook/auxiliary/symmetry.py:30-356): ``MirrorDef`` and the hooks that use it.

A ``MirrorDef`` on a device tensor is one HIP launch (``cusrl_mirror_rows``) with a differentiable backward
(``cusrl_mirror_rows_bwd``).  Its int32 index / sign table and the inverse table of its gradient are built once on the host
and uploaded once per device and input width, when a hook initialises, never during a capture.

- ``MirrorSymmetryLoss`` mirrors the minibatch's observations, runs the actor on them and evaluates both of its terms and
  their gradients in one launch (``cusrl_mirror_mse_fwd_bwd``).
- ``SymmetricDataAugmentation`` builds the ``[B, 2, ...]`` batch of the reference at objective time, from the gathered
  minibatch, in one ``cusrl_mirror_rows`` launch: the rollout pushes nothing extra and the buffer holds no doubled leaves.
- ``TransitionMirroring`` rewrites the rollout's transitions through the device mirror (shape-static, capturable).

Any other callable a user puts into ``mirror_*`` of the spec (a lambda returning a ``[K, ...]`` stack of variants, say) is
user code: it is evaluated as given, with whatever torch operations it contains.  Only ``MirrorDef`` has the device form.

- ``SymmetricArchitecture`` replaces the agent's actor with a ``SymmetricActor``, which evaluates the wrapped actor ONCE on
  the stacked ``[2B, O]`` rows (observations first, mirrored observations second: one ``cusrl_mirror_rows`` launch) and combines
  the two halves of the head's output in one launch (``cusrl_symmetric_head_fwd`` / ``_bwd`` under grad,
  ``cusrl_symmetric_head_sample`` when acting).

Not here: recurrent actors in any of the hooks.
"""

from __future__ import annotations

from collections.abc import Callable, Sequence
from dataclasses import dataclass
from typing import TypeAlias

import numpy as np
import torch
from torch import Tensor, nn

from cusrl_amd import ops
from cusrl_amd.nn.actor import Actor, ActorFactory
from cusrl_amd.nn.distribution import AdaptiveNormalDist, NormalDist
from cusrl_amd.template.hook import Hook
from cusrl_amd.utils.misc import host_form

__all__ = [
    "MirrorDef",
    "MirrorFn",
    "MirrorSymmetryLoss",
    "SymmetricActor",
    "SymmetricActorFactory",
    "SymmetricArchitecture",
    "SymmetricDataAugmentation",
    "TransitionMirroring",
]

MirrorFn: TypeAlias = Callable[[Tensor], Tensor]

_FLIP = np.int64(1) << 31


class MirrorDef:
    """Builds a mirror transform by reindexing and sign-flipping a tensor.

    The transform is applied to the last dimension of the input tensor. Values are first gathered according to
    ``destination_indices``, then the entries at positions listed in ``flipped_indices`` are multiplied by ``-1``:
    ``out[..., j] = in[..., destination_indices[j]] * (-1 if j in flipped_indices else 1)``.  The output is
    ``len(destination_indices)`` wide, which may differ from the input's width.

    On a device tensor the transform is one HIP launch, bit-exact against the reference's expression and differentiable
    (the gradient of an input column sums the output columns that read it, in increasing order).  On a CPU tensor it
    evaluates the reference's indexing expression: environments call mirrors on the host, too.

    Args:
        destination_indices (Sequence[int]):
            Indices to gather from the input tensor for each output position.
        flipped_indices (Sequence[int]):
            Output positions whose gathered values should be negated.
    """

    def __init__(self, destination_indices: Sequence[int], flipped_indices: Sequence[int]):
        self.destination_indices = destination_indices
        self.flipped_indices = flipped_indices

        self.destination = torch.tensor(destination_indices, dtype=torch.long)
        self.multiplier = torch.ones(len(destination_indices))
        self.multiplier[flipped_indices] = -1.0
        self._device_tables: dict[tuple[torch.device, int], Tensor] = {}

    def __call__(self, input: Tensor):
        if input.is_cuda:
            return _MirrorFunction.apply(input, self)
        self.destination = self.destination.to(input.device)
        self.multiplier = self.multiplier.to(dtype=input.dtype, device=input.device)
        return input[..., self.destination] * self.multiplier

    def __repr__(self):
        return f"MirrorDef(destination_indices={self.destination_indices}, flipped_indices={self.flipped_indices})"

    @property
    def output_dim(self) -> int:
        return len(self.destination_indices)

    def host_table(self, input_dim: int) -> np.ndarray:
        """The int32 table of ``include/cusrl_hip.h`` (``cusrl_mirror_rows``) for inputs ``input_dim`` wide: forward codes,
        the inverse list's offsets per input column, the inverse codes (output column | flip bit, increasing column)."""
        dest = np.asarray(self.destination.cpu(), dtype=np.int64).reshape(-1)
        c_out = dest.size
        if c_out == 0:
            raise ValueError("MirrorDef: 'destination_indices' is empty")
        dest = np.where(dest < 0, dest + input_dim, dest)
        if dest.min() < 0 or dest.max() >= input_dim:
            raise IndexError(f"MirrorDef: destination indices out of range for inputs {input_dim} wide")
        flip = np.asarray(self.multiplier.cpu()).reshape(-1) < 0
        codes = dest | np.where(flip, _FLIP, 0)
        order = np.argsort(dest, kind="stable")  # the output columns reading each input column, in increasing order
        offsets = np.zeros(input_dim + 1, dtype=np.int64)
        np.add.at(offsets, dest + 1, 1)
        offsets = np.cumsum(offsets)
        inverse = order.astype(np.int64) | np.where(flip[order], _FLIP, 0)
        return np.concatenate([codes, offsets, inverse]).astype(np.uint32).view(np.int32)

    def device_table(self, device: torch.device | str, input_dim: int) -> Tensor:
        """The table on ``device``, uploaded the first time it is asked for and cached (hooks ask at ``init``)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, int(input_dim))
        table = self._device_tables.get(key)
        if table is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self!r}: its device table for {input_dim}-wide inputs was not uploaded before the "
                                   "capture (symmetry hooks upload theirs at init)")
            table = self._device_tables[key] = torch.from_numpy(self.host_table(input_dim)).to(device)
        return table

    def device_form(self, device: torch.device | str, input_dim: int) -> tuple[Tensor, int, int]:
        """``(table, C_in, C_out)`` as ``ops.mirror_rows`` takes it."""
        return self.device_table(device, input_dim), int(input_dim), self.output_dim


class _MirrorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, mirror):
        c_in = input.shape[-1]
        form = mirror.device_form(input.device, c_in)
        src = input.reshape(-1, c_in)
        out = torch.empty(src.shape[0], form[2], dtype=torch.float32, device=input.device)
        ops.mirror_rows([(src, out, 0, form)], src.shape[0])
        ctx.table, ctx.c_in = form[0], c_in
        return out.view(*input.shape[:-1], form[2])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ops.mirror_rows_bwd(grad_out, ctx.table, ctx.c_in), None


class _MirrorSymmetryLossFunction(torch.autograd.Function):
    """(mean term, std term) of MirrorSymmetryLoss with the gradients from the forward launch."""

    @staticmethod
    def forward(ctx, mean, mirrored_mean, std, mirrored_std, table, weight):
        losses, d_mean, d_mirrored, d_std, d_mirrored_std = ops.mirror_mse_fwd_bwd(
            mean, mirrored_mean, table, weight, std, mirrored_std)
        ctx.save_for_backward(*(t for t in (d_mean, d_mirrored, d_std, d_mirrored_std) if t is not None))
        ctx.has_std = std is not None
        ctx.shapes = (mean.shape, None if std is None else std.shape)
        ctx.set_materialize_grads(False)
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mean, g_std):
        from cusrl_amd.nn.module import saved_gradients

        saved = ctx.saved_tensors
        d_mean = d_mirrored = d_std = d_mirrored_std = None
        if g_mean is not None:
            d_mean, d_mirrored = (g.view(ctx.shapes[0]) for g in saved_gradients(saved[:2], g_mean))
        if ctx.has_std and g_std is not None:
            d_std, d_mirrored_std = (g.view(ctx.shapes[1]) for g in saved_gradients(saved[2:4], g_std))
        return d_mean, d_mirrored, d_std, d_mirrored_std, None, None


def _prepare(mirror, device, input_dim: int) -> None:
    """Upload a MirrorDef's table for ``device`` now (outside any capture); other callables need nothing."""
    if isinstance(mirror, MirrorDef) and torch.device(device).type == "cuda":
        mirror.device_table(device, input_dim)


def _std_vector(std: Tensor) -> Tensor | None:
    """The ``[A]`` vector a state-independent std is a broadcast view of, if it is one."""
    row_vector = getattr(std, "_cusrl_row_vector", None)
    if row_vector is not None and std.dim() >= 2 and all(s == 0 for s in std.stride()[:-1]):
        return row_vector
    return None


class _SymmetryHook(Hook):
    mirror_observation: MirrorFn
    mirror_state: MirrorFn | None
    mirror_action: MirrorFn

    def init(self):
        spec = self.agent.environment_spec
        if spec.mirror_observation is None:
            raise ValueError("'mirror_observation' must be defined for symmetry hooks")
        self.mirror_observation = spec.mirror_observation

        if self.agent.has_state and spec.mirror_state is None:
            raise ValueError("'mirror_state' must be defined for symmetry hooks")
        self.mirror_state = spec.mirror_state

        if spec.mirror_action is None:
            raise ValueError("'mirror_action' must be defined for symmetry hooks")
        self.mirror_action = spec.mirror_action

        device = self.agent.device
        _prepare(self.mirror_observation, device, self.agent.observation_dim)
        if self.mirror_state is not None and self.agent.has_state:
            _prepare(self.mirror_state, device, self.agent.state_dim)
        _prepare(self.mirror_action, device, self.agent.action_dim)

    def _refuse_recurrent(self):
        if getattr(self.agent.actor, "is_recurrent", False):
            raise NotImplementedError(
                f"{type(self).__name__} does not support recurrent actors yet: the mirrored memory leaves and temporal "
                "batches of the reference have no device form here")

    def _device_check(self, tensor: Tensor):
        if not tensor.is_cuda:
            host_form(type(self).__name__)  # test processes without a GPU only

    @staticmethod
    def _build_mirrored(original: Tensor, mirror: MirrorFn) -> Tensor:
        mirrored = mirror(original)
        if mirrored.shape[1:] == original.shape:
            return mirrored
        if mirrored.shape[1:] == original.shape[1:]:
            return mirrored.reshape(-1, *original.shape)

        original_shape_str = ", ".join(str(s) for s in original.shape)
        raise ValueError(
            f"Mirrored tensor has incompatible shape: expected (N * {original_shape_str}) or "
            f"(N, {original_shape_str}), got {mirrored.shape}"
        )


class TransitionMirroring(_SymmetryHook):
    """Replaces collected transitions with one selected mirrored variant (symmetry.py:98-152).

    During rollout the actor consumes mirrored observations and states; the sampled action is mapped back to the
    original action space before it is returned to the environment; once the environment step completes, the stored
    transition is rewritten so that ``observation``, ``state``, ``action``, ``next_observation`` and ``next_state`` all
    correspond to the same mirrored variant.  ``index`` selects the variant when a mirror returns several; the selected
    transform is assumed to be self-inverse.  With ``MirrorDef`` mirrors every rewrite is one shape-static HIP launch, so
    a captured env step stays one graph.

    Args:
        index (int, optional):
            Index of the mirrored variant to use. Defaults to ``0``.
    """

    rollout_capture_safe = True

    def __init__(self, index: int = 0):
        if not isinstance(index, int):
            raise TypeError("'index' must be an int")
        super().__init__()
        self.index = index

    def pre_act(self, transition):
        observation = transition["observation"]
        self._device_check(observation)
        transition["observation"] = self._select_mirrored_tensor(observation, self.mirror_observation, self.index)
        if (state := transition.get("state")) is not None:
            transition["state"] = self._select_mirrored_tensor(state, self.mirror_state, self.index)

    def post_act(self, transition):
        transition["action"] = self._select_mirrored_tensor(transition["action"], self.mirror_action, self.index)

    def post_step(self, transition):
        transition["next_observation"] = self._select_mirrored_tensor(
            transition["next_observation"], self.mirror_observation, self.index)
        if (next_state := transition.get("next_state")) is not None:
            transition["next_state"] = self._select_mirrored_tensor(next_state, self.mirror_state, self.index)

    @classmethod
    def _select_mirrored_tensor(cls, original: Tensor, mirror: MirrorFn, index: int) -> Tensor:
        mirrored = cls._build_mirrored(original, mirror)
        num_symmetries = mirrored.shape[0]
        if not -num_symmetries <= index < num_symmetries:
            raise IndexError(f"Mirror index {index} is out of range for {num_symmetries} symmetry transforms")
        return mirrored[index]


class MirrorSymmetryLoss(_SymmetryHook):
    """Implements a mirror symmetry loss to facilitate symmetry in the action distribution (symmetry.py:155-231).

    Described in "Learning Symmetric and Low-Energy Locomotion",
    https://dl.acm.org/doi/abs/10.1145/3197517.3201397

    With ``MirrorDef`` mirrors on a device, the mirrored observations are one ``cusrl_mirror_rows`` launch and both terms
    with their gradients one ``cusrl_mirror_mse_fwd_bwd`` launch; autograd adds ``d mean`` to the fused PPO objective's.

    Args:
        weight (float | None):
            Scaling factor for the symmetry loss. If ``None``, the symmetry loss is not applied.
        symmetrize_action_std (bool, optional):
            Whether to symmetrize the action standard deviation. Defaults to ``False``.
    """

    def __init__(self, weight: float | None, symmetrize_action_std: bool = False):
        if weight is not None and weight < 0:
            raise ValueError("'weight' must be None or non-negative")
        super().__init__()
        self.symmetrize_action_std = symmetrize_action_std

        # Mutable attributes
        self.weight: float | None = weight
        self.register_mutable("weight")

    def init(self):
        super().init()
        self._refuse_recurrent()
        self.criterion = nn.MSELoss()

    def objective(self, metadata, batch):
        if self.weight is None:
            return None

        actor = self.agent.actor
        observation = batch["observation"]
        self._device_check(observation)
        mirrored_action_dist, _ = actor(self.mirror_observation(observation), done=batch["done"])
        curr_action_dist = batch["curr_action_dist"]
        mean, mirrored_mean = curr_action_dist["mean"], mirrored_action_dist["mean"]
        if isinstance(self.mirror_action, MirrorDef) and mean.is_cuda:
            std = mirrored_std = None
            if self.symmetrize_action_std:
                std, mirrored_std = curr_action_dist["std"], mirrored_action_dist["std"]
                vectors = _std_vector(std), _std_vector(mirrored_std)
                if vectors[0] is not None and vectors[1] is not None:
                    std, mirrored_std = vectors
                else:
                    std, mirrored_std = std.expand_as(mean), mirrored_std.expand_as(mean)
            table = self.mirror_action.device_table(mean.device, mean.shape[-1])
            mean_loss, std_loss = _MirrorSymmetryLossFunction.apply(
                mean.float(), mirrored_mean.float(), std, mirrored_std, table, float(self.weight))
            losses = {"action_mean_symmetry_loss": mean_loss}
            if self.symmetrize_action_std:
                losses["action_std_symmetry_loss"] = std_loss
            return losses

        # a user-supplied mirror callable: the reference's expression as given
        losses = {"action_mean_symmetry_loss": self.criterion(mean, self.mirror_action(mirrored_mean)) * self.weight}
        if self.symmetrize_action_std:
            losses["action_std_symmetry_loss"] = self.criterion(
                curr_action_dist["std"], self.mirror_action(mirrored_action_dist["std"]).abs()) * self.weight
        return losses


class SymmetricDataAugmentation(_SymmetryHook):
    """Augments training data by adding mirrored transitions to the batch (symmetry.py:234-356).

    Described in "Symmetry Considerations for Learning Task Symmetric Robot Policies",
    https://ieeexplore.ieee.org/abstract/document/10611493

    For each transition :math:`(s, a, r, s')` the batch also holds the mirrored :math:`(s_m, a_m, r, s'_m)`: the fields
    become ``[B, 2, ...]`` with the original first, and ``action_logp`` / ``advantage`` (``value`` / ``return`` too when
    ``augments_value``) are repeated, as in the reference.  The reference stores the ``augmented_*`` leaves at every env
    step; for a feed-forward agent they are a pure function of leaves the buffer already holds, so here they are built at
    objective time from the gathered minibatch, in one ``cusrl_mirror_rows`` launch (with ``MirrorDef`` mirrors).

    Args:
        augments_value (bool, optional):
            Whether to augment the value function with mirrored transitions. Defaults to ``True``.
    """

    _NARROW = ("action_logp", "advantage")
    _VALUE = ("value", "return")

    def __init__(self, augments_value: bool = True):
        self.augments_value = augments_value
        super().__init__(training_only=True)

    def init(self):
        super().init()
        self._refuse_recurrent()
        if not self.augments_value:
            # the reference's critic reads the augmented [B, 2, C] states too: its value loss then meets an un-repeated
            # [B, 1] return and fails on the shape inside the loss
            raise ValueError("SymmetricDataAugmentation(augments_value=False) cannot train: the critic also evaluates the "
                             "augmented [B, 2, ...] states, whose values do not match the un-augmented returns")

    def objective(self, metadata, batch):
        if metadata.get("temporal"):
            raise NotImplementedError("SymmetricDataAugmentation does not support temporal (recurrent) batches yet")
        observation = batch["observation"]
        self._device_check(observation)
        mirrored = [("observation", self.mirror_observation), ("next_observation", self.mirror_observation),
                    ("action", self.mirror_action)]
        if self.agent.has_state:
            mirrored += [("state", self.mirror_state), ("next_state", self.mirror_state)]
        repeated = [key for key in self._NARROW if batch.get(key) is not None]
        if self.augments_value:
            repeated += list(self._VALUE)
        sources = {key: batch[key] for key, _ in mirrored}
        sources.update((key, batch[key]) for key in repeated)
        device_form = observation.is_cuda and all(isinstance(mirror, MirrorDef) for _, mirror in mirrored)
        if device_form:
            augmented = self._augment_on_device(sources, mirrored, repeated)
        else:  # a user-supplied mirror callable (or a host process): the reference's expressions as given
            augmented = {key: self._build_augmented_tensor(sources[key], mirror) for key, mirror in mirrored}
            augmented.update((key, sources[key].unsqueeze(1).repeat_interleave(2, dim=1)) for key in repeated)
        for key, value in augmented.items():
            batch[key] = value

    def _augment_on_device(self, sources: dict[str, Tensor], mirrored, repeated) -> dict[str, Tensor]:
        rows = sources["observation"].shape[0]
        fields, out = [], {}
        for key, mirror in mirrored:
            src = sources[key]
            width = src.shape[-1]
            if mirror.output_dim != width:
                raise ValueError(f"Mirrored tensor has incompatible shape: expected (N * {rows}, {width}) or (N, {rows}, {width}), "
                                 f"got {(rows, mirror.output_dim)}")
            dst = torch.empty(rows, 2, width, dtype=torch.float32, device=src.device)
            flat = dst.view(rows, 2 * width)
            fields += [(src, flat, 0, None), (src, flat, width, mirror.device_form(src.device, width))]
            out[key] = dst
        for key in repeated:
            src = sources[key]
            width = src.shape[-1]
            dst = torch.empty(rows, 2, width, dtype=torch.float32, device=src.device)
            flat = dst.view(rows, 2 * width)
            fields += [(src, flat, 0, None), (src, flat, width, None)]
            out[key] = dst
        context = getattr(self.agent, "step_context", None)
        branch = getattr(context, "critic_stream", None)
        main = torch.cuda.current_stream()
        if branch is not None and getattr(context, "batch_on_branch", False):
            main.wait_stream(branch)  # the step's rows were gathered on the critic's stream
        for start in range(0, len(fields), ops._native.MAX_MIRROR_FIELDS):
            ops.mirror_rows(fields[start:start + ops._native.MAX_MIRROR_FIELDS], rows)
        if branch is not None:
            branch.wait_stream(main)  # the critic reads the augmented rows on its own stream (ValueLoss)
        return out

    @classmethod
    def _build_augmented_tensor(cls, original: Tensor, mirror: MirrorFn, augmentation_dim: int = 1) -> Tensor:
        mirrored = cls._build_mirrored(original, mirror).movedim(0, augmentation_dim)
        return torch.cat([original.unsqueeze(augmentation_dim), mirrored], dim=augmentation_dim)


class SymmetricArchitecture(_SymmetryHook):
    """Enforces a symmetric architecture on the agent's actor (symmetry.py:359-377).

    Described in "On Learning Symmetric Locomotion",
    https://dl.acm.org/doi/abs/10.1145/3359566.3360070

    This hook wraps the agent's original actor with a ``SymmetricActor`` during the initialization phase, ensuring that the
    policy is strictly symmetric.  It contributes no objective: the stock four objective hooks stay one fused launch.
    """

    def pre_init(self, agent):
        super().pre_init(agent)
        agent.actor_factory = SymmetricActorFactory(
            agent.actor_factory.backbone_factory,
            agent.actor_factory.distribution_factory,
            agent.actor_factory.latent_dim,
            mirror_observation=agent.environment_spec.mirror_observation,
            mirror_action=agent.environment_spec.mirror_action,
        )


@dataclass(slots=True)
class SymmetricActorFactory(ActorFactory):
    mirror_observation: MirrorFn | None = None
    mirror_action: MirrorFn | None = None

    def __call__(self, input_dim: int | None = None, output_dim: int | None = None):
        actor = ActorFactory.__call__(self, input_dim, output_dim)
        assert self.mirror_observation is not None, "'mirror_observation' must be defined"
        assert self.mirror_action is not None, "'mirror_action' must be defined"
        return SymmetricActor(actor, mirror_observation=self.mirror_observation, mirror_action=self.mirror_action)


class _SymmetricHeadFunction(torch.autograd.Function):
    """``(mean, std) [B, A]`` of a symmetric actor from the stacked head outputs, one launch each way.  ``bias``: the head's bias,
    which ``mean2`` already contains as a constant (``detach_mean_bias``); it is an input only so that its gradient comes from
    here — the column sums of ``d_mean2`` with the two halves added row by row, exactly 0 for a column that mirrors onto itself
    with a flip, as in the reference's two passes (one fp32 sum over the 2B stacked rows leaves a residue that Adam amplifies)."""

    @staticmethod
    def forward(ctx, mean2, std2, table, bias):
        mean, std = ops.symmetric_head_fwd(mean2, std2, table)
        ctx.save_for_backward(std2)
        ctx.table = table
        ctx.set_materialize_grads(False)
        return mean, std

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mean, g_std):
        g_std = g_std if ctx.needs_input_grad[1] else None
        want_bias = ctx.needs_input_grad[3] and g_mean is not None
        g_mean = g_mean if ctx.needs_input_grad[0] or want_bias else None
        if g_mean is None and g_std is None:
            return None, None, None, None
        (std2,) = ctx.saved_tensors
        d_mean2, d_std2, d_bias = ops.symmetric_head_bwd(g_mean, g_std, std2, ctx.table, want_bias=want_bias)
        return (d_mean2 if ctx.needs_input_grad[0] else None), d_std2, None, d_bias


class SymmetricActor(Actor):
    """An actor whose action distribution is strictly mirror-symmetric (symmetry.py:396-508):
    ``mean = (mean(o) + M_a(mean(M_o(o)))) / 2`` and ``std = (std(o) + |M_a(std(M_o(o)))|) / 2``.

    The reference calls the wrapped actor twice.  A feed-forward network is row-independent, so here it is evaluated ONCE
    on the stacked ``[2B, O]`` rows (observations first, mirrored observations second, written by one ``cusrl_mirror_rows``
    launch): every layer is used once per graph and sees an ordinary batch of ``2B`` rows.  The halves of the head's output are
    combined by ``cusrl_symmetric_head_fwd`` (backward: ``cusrl_symmetric_head_bwd``); acting without a gradient ends in
    ``cusrl_symmetric_head_sample`` instead, behind ``cusrl_mlp2_forward`` where that takes the wrapped actor: three launches
    per act step.  ``intermediate_repr`` carries the reference's keys as views of the stacked tensors' halves.

    Only ``MirrorDef`` mirrors have the device form.  Any other callable is user code and is evaluated as given, through the
    reference's torch expressions; so are operands the kernels do not take (a CPU tensor in a test process, an action wider than
    the kernels' limit).  Recurrent actors are not supported, as in the other symmetry hooks: ``memory`` is None in and out.
    """

    def __init__(self, wrapped: Actor, mirror_observation: MirrorFn, mirror_action: MirrorFn):
        super().__init__(wrapped.backbone, wrapped.distribution)
        if not isinstance(self.distribution, (NormalDist, AdaptiveNormalDist)):
            raise ValueError("SymmetricActor can only be used with Normal distributions")
        if self.is_recurrent:
            raise NotImplementedError("SymmetricActor does not support recurrent actors yet: the mirrored memory of the "
                                      "reference has no device form here")
        for name, mirror in (("mirror_observation", mirror_observation), ("mirror_action", mirror_action)):
            if not isinstance(mirror, MirrorDef) and not callable(mirror):
                raise TypeError(f"SymmetricActor: '{name}' must be a MirrorDef (or a callable, which is evaluated as given), "
                                f"got {type(mirror).__name__}")
        self.wrapped = wrapped
        self.mirror_observation = mirror_observation
        self.mirror_action = mirror_action

    def clear_intermediate_repr(self):
        super().clear_intermediate_repr()
        self.wrapped.clear_intermediate_repr()

    # ------------------------------------------------------------------ the stacked pass
    def _device_form(self, observation: Tensor) -> bool:
        if not (isinstance(self.mirror_observation, MirrorDef) and isinstance(self.mirror_action, MirrorDef)):
            return False
        if not observation.is_cuda:
            host_form(type(self).__name__)  # test processes without a GPU only
            return False
        rows = observation.numel() // max(observation.shape[-1], 1)
        return (observation.dtype == torch.float32 and not torch.is_autocast_enabled("cuda")
                and ops.symmetric_head_supported(rows, self.output_dim))

    def _stack(self, observation: Tensor, device_form: bool) -> Tensor:
        """``[2B, O]``: the observations, then their mirror images."""
        if not device_form:
            return torch.cat([observation, self.mirror_observation(observation)], dim=0)
        rows, width = observation.shape
        if self.mirror_observation.output_dim != width:
            raise ValueError(f"SymmetricActor: 'mirror_observation' gives {self.mirror_observation.output_dim} columns for "
                             f"observations {width} wide")
        stacked = torch.empty(2 * rows, width, dtype=torch.float32, device=observation.device)
        ops.mirror_rows([(observation, stacked[:rows], 0, None),
                         (observation, stacked[rows:], 0, self.mirror_observation.device_form(observation.device, width))], rows)
        return stacked

    def _symmetric_pass(self, observation: Tensor, backbone_kwargs, distribution_kwargs, sample: bool):
        """``(action_dist, (action, logp) | None)``; fills ``intermediate_repr``."""
        device_form = self._device_form(observation)
        lead = observation.shape[:-1]
        if device_form and observation.dim() != 2:
            observation = observation.reshape(-1, observation.shape[-1])
        stacked = self._stack(observation, device_form)
        rows = stacked.shape[0] // 2
        wrapped = self.wrapped
        wrapped.intermediate_repr.clear()
        grad = torch.is_grad_enabled()
        bias = None  # the head's bias when the combine differentiates it (see _SymmetricHeadFunction)
        layers = wrapped._fused_layers(stacked, None, backbone_kwargs, distribution_kwargs) if device_form and not grad else None
        if layers is not None:  # no gradient asked for: backbone and head over the 2B rows as one launch, no sampling epilogue
            mean2 = ops.mlp2_forward(stacked, layers)
            std2 = self.distribution.std_vector()
            std_rows = std2.expand(2 * rows, -1)
        else:
            head_bias = self.distribution.mean_head.bias
            if device_form and grad and head_bias is not None and head_bias.requires_grad:
                bias, distribution_kwargs = head_bias, {**(distribution_kwargs or {}), "detach_mean_bias": True}
            dist2, _ = wrapped(stacked, memory=None, backbone_kwargs=backbone_kwargs, distribution_kwargs=distribution_kwargs)
            mean2, std_rows = dist2["mean"], dist2["std"]
            std2 = _std_vector(std_rows)
            if std2 is None:
                std2 = std_rows
        sampled = None
        if device_form:
            table = self.mirror_action.device_table(stacked.device, self.output_dim)
            mean2, std2 = mean2.float(), std2.float()
            if sample and not grad:
                # eps as the unfused path draws it: one [B, A] normal_() from torch's generator (distribution.py _Normal)
                eps = torch.empty(rows, self.output_dim, dtype=torch.float32, device=stacked.device).normal_()
                action, logp, mean, std = ops.symmetric_head_sample(mean2, std2, table, eps)
                sampled = (action.view(*lead, -1), logp.view(*lead, 1))
            elif grad and (mean2.requires_grad or std2.requires_grad or bias is not None):
                mean, std = _SymmetricHeadFunction.apply(mean2, std2, table, bias)
            else:
                mean, std = ops.symmetric_head_fwd(mean2, std2, table)
            mean, std = mean.view(*lead, -1), std.view(*lead, -1)
        else:  # the reference's expressions as given
            mean = (mean2[:rows] + self.mirror_action(mean2[rows:])) / 2
            std = (std_rows[:rows] + self.mirror_action(std_rows[rows:]).abs()) / 2
        action_dist = {"mean": mean, "std": std}
        if sample and sampled is None:
            sampled = self.distribution.sample_from_dist(action_dist)

        representation = self.intermediate_repr
        halves = {key: (value[:rows], value[rows:]) for key, value in wrapped.intermediate_repr.items()
                  if isinstance(value, Tensor) and value.shape[:1] == (2 * rows,)}
        representation["original.action_dist"] = {"mean": mean2[:rows], "std": std_rows[:rows]}
        representation.update((f"original.{key}", pair[0]) for key, pair in halves.items())
        representation["mirrored.observation"] = stacked[rows:]
        representation["mirrored.action_dist"] = {"mean": mean2[rows:], "std": std_rows[rows:]}
        representation.update((f"mirrored.{key}", pair[1]) for key, pair in halves.items())
        return action_dist, sampled

    def forward(self, observation: Tensor, memory=None, done: Tensor | None = None, backbone_kwargs=None,
                distribution_kwargs=None, forward_type: str | None = "forward", deterministic: bool = False):
        """As ``Actor.forward``; ``done`` only matters to a recurrent backbone and is not passed on."""
        if memory is not None:
            raise NotImplementedError("SymmetricActor does not support recurrent actors yet")
        if forward_type == "act_deterministic":
            forward_type, deterministic = "act", True
        if forward_type not in ("forward", "explore", "act"):
            raise ValueError(f"Unsupported 'forward_type' value: {forward_type!r}")
        sample = forward_type != "forward" and not deterministic
        action_dist, sampled = self._symmetric_pass(observation, backbone_kwargs, distribution_kwargs, sample)
        if forward_type == "forward":
            return action_dist, None
        if deterministic:
            # (determine(o) + M(determine(M(o)))) / 2 of the reference: for a Normal that is the combined mean
            action = action_dist["mean"]
            sampled = (action, self.distribution.compute_logp(action_dist, action))
        if forward_type == "act":
            return sampled[0], None
        return action_dist, sampled, None

    def step_memory(self, observation, memory=None, **kwargs):
        return None  # (feed-forward: None in, None out)

    def reset_memory(self, memory, done=None):
        return
