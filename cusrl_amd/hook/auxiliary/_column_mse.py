"""``weight * nn.MSELoss()(prediction, target[..., indices])`` as the privileged-information hooks evaluate it (estimation.py,
representation.py, distillation.py of the reference): on a device, loss AND d loss / d prediction from one pass over the
prediction with the target — a buffer leaf of the minibatch — read in place through its row pitch and an int32 column table
(``cusrl_column_mse_fwd_bwd``), instead of an index gather, sub / square / mean, the multiply by the weight and fill /
mse_backward / mul behind them."""

from __future__ import annotations

import torch
from torch import Tensor, nn

from cusrl_amd.utils.misc import host_form

__all__ = ["ColumnSelection", "weighted_column_mse"]


class ColumnSelection:
    """``indices`` (a slice, an int list or an index tensor) applied to the last dimension of a ``width``-wide leaf.  The
    int32 device table is uploaded by :meth:`prepare` — hooks call it at ``init``, never during a capture; ``slice(None)``
    has none (the kernel then reads columns ``0..K-1``)."""

    def __init__(self, indices, width: int):
        from cusrl_amd import ops

        self.indices, self.width = indices, int(width)
        self.columns = ops.resolve_columns(indices, width)  # host int32 vector, or None: every column
        self.dim = self.width if self.columns is None else int(self.columns.numel())
        self._tables: dict[torch.device, Tensor] = {}

    def torch_index(self):
        """What ``target[..., index]`` takes: the indices as given (a negative-step slice, which torch refuses, as its columns)."""
        if isinstance(self.indices, slice) and (self.indices.step or 1) < 0:
            return self.columns.long()
        return self.indices

    def prepare(self, device) -> None:
        device = torch.device(device)
        if self.columns is None or device.type != "cuda" or device in self._tables:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"the column table of {self.indices!r} was not uploaded before the capture (hooks upload theirs at init)")
        from cusrl_amd import ops

        self._tables[device] = ops.column_table(self.indices, self.width, device)

    def table(self, device) -> Tensor | None:
        if self.columns is None:
            return None
        self.prepare(device)
        return self._tables[torch.device(device)]


class _ColumnMseFunction(torch.autograd.Function):
    """The weighted loss with the target constant; the gradient wrt the prediction comes from the forward launch."""

    @staticmethod
    def forward(ctx, prediction, target, columns, weight):
        from cusrl_amd import ops

        loss, grad = ops.column_mse_fwd_bwd(prediction, target, columns, weight)
        ctx.save_for_backward(grad)
        ctx.shape = prediction.shape
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        from cusrl_amd.nn.module import saved_gradients

        (grad,) = saved_gradients(ctx.saved_tensors, grad_loss)
        return grad.view(ctx.shape), None, None, None


def weighted_column_mse(what: str, criterion: nn.Module, prediction: Tensor, target: Tensor, selection: ColumnSelection | None,
                        weight: float) -> Tensor:
    """``criterion(prediction, target[..., indices]) * weight``.  ``selection``: None = the whole target.  The HIP form is
    taken for a device fp32 prediction against an fp32 target of the same leading shape that needs no gradient, under the
    stock mean ``nn.MSELoss``; a user-supplied criterion (and a process without a GPU, ``host_form``) keeps the reference's
    torch expression."""
    if (prediction.is_cuda and type(criterion) is nn.MSELoss and criterion.reduction == "mean"
            and prediction.dtype == torch.float32 and target.dtype == torch.float32 and not target.requires_grad
            and target.is_cuda and prediction.dim() >= 1 and prediction.shape[:-1] == target.shape[:-1]
            and (selection is None or selection.width == target.shape[-1])):
        columns = None if selection is None else selection.table(prediction.device)
        if prediction.shape[-1] == (target.shape[-1] if columns is None else columns.numel()):
            return _ColumnMseFunction.apply(prediction, target, columns, float(weight))
    if not prediction.is_cuda:
        host_form(what)  # test processes without a GPU only
    index = slice(None) if selection is None else selection.torch_index()
    if isinstance(index, Tensor):
        index = index.to(target.device)
    return criterion(prediction, target[..., index]) * weight
