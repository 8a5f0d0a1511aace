"""The last ``stack_size`` observations of every row as one observation (gymnasium's ``FrameStackObservation``, oldest first):
what gives a feed-forward policy the velocities it cannot see, and what stands in front of a ``DeployedPolicy`` trained on
stacked observations — ``policy(stacker(observation))`` — done by the code that did it in training (``environment.FrameStack``
keeps its history through the same two kernels, ``csrc/frame_stack.hip``; DESIGN.md §7, "Frame stacking").

``stacker(observation [B, K0]) -> [B, S * K]`` with ``K = len(columns)`` (``K0`` without ``columns``); the history ``[B, S, K]`` is
allocated at the first call and updated in place.  A row's first observation — the first call, and the call after the row was
marked by ``reset(done)`` or by a ``done=`` — fills its history by ``padding_type``: ``"reset"`` repeats it in every slot,
``"zero"`` puts zeros in front of it.

On an MI355X a contiguous fp32 ``[B, K0]`` input costs exactly one ``cusrl_frame_stack_push`` launch.  Any other input evaluates
the torch expression in fp32; on the CPU that is a host form (``utils.misc.host_form``)."""

from __future__ import annotations

import torch
from torch import Tensor, nn

__all__ = ["ObservationStacker"]


class ObservationStacker(nn.Module):
    def __init__(self, observation_dim: int, stack_size: int, padding_type: str = "reset", columns=None):
        super().__init__()
        from cusrl_amd import ops

        self.observation_dim, self.stack_size = int(observation_dim), int(stack_size)
        if self.observation_dim < 1:
            raise ValueError(f"observation_dim must be at least 1; got {observation_dim}")
        if self.stack_size < 1:
            raise ValueError(f"stack_size must be at least 1; got {stack_size}")
        ops.frame_stack_padding(padding_type)
        self.padding_type = padding_type
        table = ops.frame_stack_columns(columns, self.observation_dim, "cpu")
        self.columns: tuple[int, ...] | None = None if table is None else tuple(table.tolist())
        self.width = self.observation_dim if table is None else len(self.columns)
        self.output_dim = self.stack_size * self.width
        self._table: Tensor | None = None
        self._history: Tensor | None = None
        self._fresh: Tensor | None = None

    # ---- history
    @property
    def history(self) -> Tensor | None:
        """``[B, S, K]``, slot 0 the oldest (None before the first call); assign None to start over."""
        return self._history

    @history.setter
    def history(self, value) -> None:
        if value is not None:
            raise ValueError("the history is written by the stacker itself; assign None to start over")
        self._history = self._fresh = None

    def reset(self, done: Tensor | None = None) -> None:
        """Mark the rows where ``done`` (``[B]`` or ``[B, 1]``, bool) is set — every row when ``done`` is None: their next
        observation starts a fresh history by the padding rule."""
        if self._fresh is None:
            return
        if done is None:
            self._fresh.fill_(True)
        else:
            self._fresh.logical_or_(self._done(done, self._fresh.shape[0], self._fresh.device))

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

    def _ensure(self, rows: int, device) -> None:
        from cusrl_amd import ops

        if self._history is None:
            self._history = torch.zeros(rows, self.stack_size, self.width, dtype=torch.float32, device=device)
            self._fresh = torch.ones(rows, dtype=torch.bool, device=device)
        elif self._history.shape[0] != rows:
            raise ValueError(f"The stacker's history holds {self._history.shape[0]} rows, the observation {rows}; assign "
                             "'history = None' to start over with another batch size")
        elif self._history.device != device:
            self._history, self._fresh = self._history.to(device), self._fresh.to(device)
        if self.columns is not None and (self._table is None or self._table.device != device):
            self._table = ops.frame_stack_columns(self.columns, self.observation_dim, device)

    def _apply(self, fn, *args, **kwargs):
        result = super()._apply(fn, *args, **kwargs)
        if self._history is not None:
            self._history, self._fresh = fn(self._history), fn(self._fresh)
        return result

    # ---- evaluation
    @torch.no_grad()
    def forward(self, observation: Tensor, done: Tensor | None = None) -> Tensor:
        """The stacked observation for ``observation [B, K0]``.  ``done`` (``[B]`` or ``[B, 1]`` bool): the envs that finished
        WITH this observation — their rows are marked behind the call, as a ``reset(done)`` after it would."""
        from cusrl_amd import ops

        if not isinstance(observation, Tensor) or observation.dim() != 2 or observation.shape[1] != self.observation_dim:
            found = tuple(observation.shape) if isinstance(observation, Tensor) else type(observation).__name__
            raise ValueError(f"'observation' must be a [B, {self.observation_dim}] tensor; got {found}")
        self._ensure(observation.shape[0], observation.device)
        if done is not None:
            done = self._done(done, observation.shape[0], observation.device)
        if ops.frame_stack_supported(self._history, observation, self._table):
            stacked = ops.frame_stack_push(self._history, observation, self._table, self._fresh, self.padding_type)
        else:
            if not observation.is_cuda:
                from cusrl_amd.utils.misc import host_form

                host_form("ObservationStacker")
            stacked = self._forward_torch(observation.float())
        if done is not None:
            self._fresh.copy_(done)  # (every flag was cleared by the push)
        return stacked

    def _forward_torch(self, x: Tensor) -> Tensor:
        history, fresh = self._history, self._fresh
        if self.columns is not None:
            x = x[:, list(self.columns)]
        newest = x.unsqueeze(1)
        shifted = torch.cat((history[:, 1:], newest), 1)
        front = newest.expand(-1, self.stack_size - 1, -1) if self.padding_type == "reset" else torch.zeros_like(history[:, 1:])
        history.copy_(torch.where(fresh.view(-1, 1, 1), torch.cat((front, newest), 1), shifted))
        fresh.fill_(False)
        return history.reshape(history.shape[0], -1).clone()

    def extra_repr(self) -> str:
        return (f"observation_dim={self.observation_dim}, stack_size={self.stack_size}, padding_type={self.padding_type!r}, "
                f"columns={None if self.columns is None else list(self.columns)}, output_dim={self.output_dim}")
