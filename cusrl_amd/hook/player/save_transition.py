"""Record what the play loop saw into ``.npz`` files (counterpart of cusrl/hook/player/save_transition.py:17-88).

Arguments, file naming, shard numbering and the saved arrays (``[steps, N, ...]`` per key, the transition's dtypes) are the
reference's.  How the data reaches the host is not: the reference converts every key of every step with ``to_numpy`` — one
synchronising device->host copy each.  Here ``step`` keeps a detached device clone per key (device-to-device, nothing waits) and
``flush`` stacks each key on the device and copies it to the host once.  CPU tensors and NumPy arrays take the reference's path."""

from __future__ import annotations

import os
from collections import defaultdict
from collections.abc import Iterable
from datetime import datetime
from pathlib import Path
from typing import Any

import numpy as np
import torch

from cusrl_amd.template.player import Player, PlayerHook
from cusrl_amd.utils.misc import to_numpy

__all__ = ["SaveTransition"]


class SaveTransition(PlayerHook):
    DEFAULT_KEYS = ("observation", "reward", "terminated", "truncated", "action")

    def __init__(self, output_path: str | os.PathLike | None = None, keys: Iterable[str] = DEFAULT_KEYS,
                 save_interval: int | None = None):
        if output_path is None:
            output_path = Path(f"transition_{datetime.now().strftime('%Y%m%d_%H%M%S')}.npz")
        else:
            output_path = Path(output_path)
            if output_path.suffix != ".npz":
                output_path = Path(f"{output_path}.npz")
        self.output_path: Path = output_path
        self.keys: tuple[str, ...] = tuple(keys)
        self.save_interval: int | None = save_interval
        self.shard_index: int = 0
        self.buffer: defaultdict[str, list[Any]] = defaultdict(list)

    def init(self, player: Player):
        super().init(player)
        if self.save_interval is not None and self.save_interval <= 0:
            raise ValueError("'save_interval' must be a positive integer or None")
        self.shard_index = 0
        self.buffer.clear()

    def step(self, step: int, transition: dict[str, Any]):
        for key in self.keys:
            value = transition[key]
            if isinstance(value, torch.Tensor) and value.is_cuda:
                self.buffer[key].append(value.detach().clone())
            else:
                self.buffer[key].append(to_numpy(value))
        if self.save_interval is not None and (step + 1) % self.save_interval == 0:
            self.flush()

    def close(self):
        self.flush()

    def flush(self):
        if not self.buffer:
            return
        arrays = {key: self._stack(values) for key, values in self.buffer.items()}
        output_path = self.output_path
        if self.save_interval is not None:
            output_path = output_path.with_name(f"{output_path.stem}_{self.shard_index:06d}.npz")
        output_path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(output_path, **arrays)
        self.shard_index += 1
        self.buffer.clear()

    @staticmethod
    def _stack(values: list) -> np.ndarray:
        if all(isinstance(value, torch.Tensor) for value in values):
            return torch.stack(values, dim=0).cpu().numpy()  # one device-to-host copy for the key
        return np.stack([to_numpy(value) for value in values], axis=0)
