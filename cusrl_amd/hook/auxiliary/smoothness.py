"""Action smoothness (counterpart of cusrl/hook/auxiliary/smoothness.py:14-109): the first- and second-order differences of the
action mean along time, cut at episode ends, as weighted mean absolute values.

On a ``[T, B, A]`` fp32 device mean both terms and their gradients come from ONE C-ABI call
(``cusrl_action_smoothness_fwd_bwd``): no padded copy of the minibatch, no boolean-mask gather, no host read of a sequence
count.  The weights are ``[A]`` device vectors the kernel reads, uploaded at ``init`` and refreshed in place by
``update_attribute`` — a captured step sees a changed weight without a new capture.

In closed form (``done[t, b]`` ends an episode at ``t``, that step included; ``done[T-1]`` never matters):

- first order, ``1 <= t < T``: the pair ``(t-1, t)`` is valid iff ``!done[t-1, b]``; ``d1 = mean[t] - mean[t-1]``;
- second order, ``2 <= t < T``: the triple is valid iff ``!done[t-2, b] && !done[t-1, b]``;
  ``d2 = -mean[t-2] + 2 mean[t-1] - mean[t]``;
- ``loss_k = sum_valid sum_a w_k[a] |d_k| / (n_k A)``.

Anything else (a CPU tensor in a test process, ``mean.ndim > 3``, another dtype) evaluates the same selection as a torch
expression on shifted ``done`` masks.
"""

from __future__ import annotations

from collections.abc import Sequence

import torch
from torch import Tensor

from cusrl_amd import ops
from cusrl_amd.template.hook import Hook
from cusrl_amd.utils.misc import host_form

__all__ = ["ActionSmoothnessLoss"]

Weight = float | Sequence[float] | None


class _ActionSmoothnessFunction(torch.autograd.Function):
    """(first-order term, second-order term) with the gradients from the forward call: one saved ``[T, B, A]`` plane per term."""

    @staticmethod
    def forward(ctx, mean, done, w1, w2):
        losses, _, d_mean = ops.action_smoothness_fwd_bwd(mean, done, w1, w2)
        ctx.save_for_backward(d_mean)
        ctx.planes = (None if w1 is None else 0, None if w2 is None else int(w1 is not None))
        ctx.shape = mean.shape
        ctx.set_materialize_grads(False)
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_1st, g_2nd):
        from cusrl_amd.nn.module import saved_gradients

        (d_mean,) = ctx.saved_tensors
        total = None
        for plane, incoming in zip(ctx.planes, (g_1st, g_2nd)):
            if plane is None or incoming is None:
                continue
            (share,) = saved_gradients((d_mean[plane],), incoming)
            total = share if total is None else total + share
        return (None if total is None else total.view(ctx.shape)), None, None, None


def _masked_mean_abs(difference: Tensor, valid: Tensor, weight: Tensor) -> Tensor:
    return (weight * difference[valid].abs()).mean()


class ActionSmoothnessLoss(Hook):
    """Penalizes non-smooth actions in temporal sequences.

    This hook calculates a loss based on the 1st and/or 2nd order differences of the action sequence, effectively
    penalizing high action velocities and accelerations.  The differences are those of a 1D convolution along time with
    the fixed kernels ``[-1, 1]`` (velocity) and ``[-1, 2, -1]`` (acceleration), taken inside every episode of the temporal
    minibatch.

    Args:
        weight_1st_order (float | Sequence[float] | None, optional):
            Weight for the 1st order smoothness loss. Could be a scalar or a sequence matching the action dimension.
            Defaults to ``None``.
        weight_2nd_order (float | Sequence[float] | None, optional):
            Weight for the 2nd order smoothness loss. Could be a scalar or a sequence matching the action dimension.
            Defaults to ``None``.
    """

    def __init__(self, weight_1st_order: Weight = None, weight_2nd_order: Weight = None):
        super().__init__()

        # Mutable attributes
        self.weight_1st_order: Weight = weight_1st_order
        self.weight_2nd_order: Weight = weight_2nd_order
        self.register_mutable("weight_1st_order")
        self.register_mutable("weight_2nd_order")

        # Runtime attributes
        self._weight1_tensor: Tensor | None = None
        self._weight2_tensor: Tensor | None = None
        self._device_weights: dict[tuple[str, torch.device, int], Tensor] = {}

    def init(self):
        self._weight1_tensor = None if self.weight_1st_order is None else self.agent.to_tensor(self.weight_1st_order)
        self._weight2_tensor = None if self.weight_2nd_order is None else self.agent.to_tensor(self.weight_2nd_order)
        device, action_dim = getattr(self.agent, "device", None), getattr(self.agent, "action_dim", None)
        if device is not None and action_dim is not None and torch.device(device).type == "cuda":
            device = torch.empty(0, device=device).device  # (with its index)
            for name in ("weight_1st_order", "weight_2nd_order"):
                self._device_weight(name, device, int(action_dim))

    def _device_weight(self, name: str, device: torch.device, action_dim: int) -> Tensor | None:
        """The ``[A]`` fp32 device vector of a weight (a scalar repeated), uploaded the first time it is asked for — at
        ``init`` — and kept: the kernel reads it, ``update_attribute`` rewrites it in place."""
        value = getattr(self, name)
        if value is None:
            return None
        key = (name, device, action_dim)
        vector = self._device_weights.get(key)
        if vector is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self.name}: the device vector of '{name}' was not uploaded before the capture "
                                   "(the hook uploads it at init)")
            vector = self._device_weights[key] = self._host_vector(name, value, action_dim).to(device)
        return vector

    @staticmethod
    def _host_vector(name: str, value, action_dim: int) -> Tensor:
        host = torch.as_tensor(value, dtype=torch.float32, device="cpu").detach()
        if host.dim() > 1 or (host.dim() == 1 and host.numel() != action_dim):
            raise ValueError(f"'{name}' must be a scalar or a sequence of {action_dim} values, got shape {tuple(host.shape)}")
        return host.expand(action_dim).contiguous()

    def objective(self, metadata, batch):
        action_mean = batch["curr_action_dist"]["mean"]
        if action_mean.ndim == 2:
            raise ValueError("Expected batch to be temporal.")
        if (seq_len := action_mean.size(0)) < 3:
            raise ValueError(f"Expected sequences to have at least 3 time steps, but got {seq_len}.")
        if self.weight_1st_order is None and self.weight_2nd_order is None:
            return {}

        done = batch["done"]
        if action_mean.is_cuda and action_mean.ndim == 3 and action_mean.dtype == torch.float32:
            device, action_dim = action_mean.device, action_mean.size(-1)
            first, second = _ActionSmoothnessFunction.apply(
                action_mean, done, self._device_weight("weight_1st_order", device, action_dim),
                self._device_weight("weight_2nd_order", device, action_dim))
            losses = {}
            if self.weight_1st_order is not None:
                losses["action_smoothness_1st_order_loss"] = first
            if self.weight_2nd_order is not None:
                losses["action_smoothness_2nd_order_loss"] = second
            return losses

        if not action_mean.is_cuda:
            host_form(type(self).__name__)  # test processes without a GPU only
        return self._torch_expression(action_mean, done)

    def _torch_expression(self, action_mean: Tensor, done: Tensor) -> dict[str, Tensor]:
        """The reference's selection without its padded layout: a pair / triple lies inside one of the sequences that
        ``split_and_pad_sequences`` cuts exactly when no ``done`` is set before its last step."""
        open_step = ~done.reshape(done.shape[:2]).bool()  # [T, B]: the episode goes on after step t
        losses = {}
        if self.weight_1st_order is not None:
            weight = self._expression_weight(self._weight1_tensor, self.weight_1st_order, action_mean)
            first_order = action_mean[1:] - action_mean[:-1]
            losses["action_smoothness_1st_order_loss"] = _masked_mean_abs(first_order, open_step[:-1], weight)
        if self.weight_2nd_order is not None:
            weight = self._expression_weight(self._weight2_tensor, self.weight_2nd_order, action_mean)
            second_order = -action_mean[:-2] + 2.0 * action_mean[1:-1] - action_mean[2:]
            losses["action_smoothness_2nd_order_loss"] = _masked_mean_abs(
                second_order, open_step[:-2] & open_step[1:-1], weight)
        return losses

    @staticmethod
    def _expression_weight(tensor: Tensor | None, value, like: Tensor) -> Tensor:
        if tensor is None:  # (a hook used without init)
            tensor = torch.as_tensor(value, dtype=torch.float32)
        return tensor.to(device=like.device)

    def update_attribute(self, name, value):
        super().update_attribute(name, value)
        if name not in ("weight_1st_order", "weight_2nd_order"):
            return
        tensor = None if value is None else self.agent.to_tensor(value)
        if name == "weight_1st_order":
            self._weight1_tensor = tensor
        else:
            self._weight2_tensor = tensor
        for key, vector in list(self._device_weights.items()):
            if key[0] != name:
                continue
            if value is None:
                del self._device_weights[key]
            else:  # in place: a captured launch keeps reading this address
                vector.copy_(self._host_vector(name, value, key[2]))
