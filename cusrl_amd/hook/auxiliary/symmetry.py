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

Not here: ``SymmetricArchitecture`` / ``SymmetricActor`` (the act path fuses the head's bias add, sampling and log-prob into
one launch; a symmetric actor needs its own design) and recurrent actors in either hook.
"""

from __future__ import annotations

from collections.abc import Callable, Sequence
from typing import TypeAlias

import numpy as np
import torch
from torch import Tensor, nn

from cusrl_amd import ops
from cusrl_amd.template.hook import Hook
from cusrl_amd.utils.misc import host_form

__all__ = [
    "MirrorDef",
    "MirrorFn",
    "MirrorSymmetryLoss",
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
