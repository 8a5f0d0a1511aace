"""Finding a training run's checkpoints again (counterpart of cusrl/template/trial.py:15-133).

``Trial(path)`` takes an experiment directory (``Env_Algo/`` — its ``latest`` symlink is followed), a trial directory (the one with
``ckpt/`` in it; the newest ``ckpt_{i}.pt`` is chosen) or one checkpoint file, and gives the trial's home, name, the experiment /
environment / algorithm names parsed from the parent directory (``Env_Algo`` or the legacy ``Env:Algo``, else None), every saved
iteration and the metadata of ``info/trial/metadata.json`` ({} when absent)."""

from __future__ import annotations

import json
import os
import re
from pathlib import Path
from typing import Any

import torch

__all__ = ["Trial"]

_CKPT_FILENAME = re.compile(r"^ckpt_(\d+)\.pt$")


class Trial:
    def __init__(self, path: str | os.PathLike, verbose: bool = True):
        trial_path = Path(path)
        if not trial_path.exists():
            raise FileNotFoundError(f"Path '{trial_path}' does not exist")
        if trial_path.is_dir():
            self.home: Path = trial_path.absolute()
            if (self.home / "latest").is_symlink():
                self.home = (self.home / "latest").resolve()
            if not (self.home / "ckpt").is_dir():
                raise FileNotFoundError(f"'{path}' is not a valid trial directory")
            self.all_iterations = self._search_ckpt(self.home / "ckpt")
            if not self.all_iterations:
                raise FileNotFoundError(f"No checkpoint files found in '{self.home / 'ckpt'}'")
            self.iteration: int = max(self.all_iterations)
        else:
            if not self._is_checkpoint_file(trial_path):
                raise ValueError(f"'{trial_path}' is not a valid checkpoint file")
            self.home = trial_path.parent.parent.absolute()
            self.all_iterations = self._search_ckpt(self.home / "ckpt")
            self.iteration = self._get_ckpt_iteration(trial_path)

        self.name: str = self.home.name
        self.experiment_name: str | None = self.home.parent.name
        self.environment_name: str | None
        self.algorithm_name: str | None
        if self.experiment_name.count("_") == 1:
            self.environment_name, self.algorithm_name = self.experiment_name.split("_")
        elif self.experiment_name.count(":") == 1:
            self.environment_name, self.algorithm_name = self.experiment_name.split(":")
        else:  # the directory does not follow either naming convention
            self.environment_name = self.algorithm_name = self.experiment_name = None
        self.info_dir: Path = self.home / "info"
        self.metadata_path: Path = self.info_dir / "trial/metadata.json"
        self.checkpoint_path: Path = self.home / f"ckpt/ckpt_{self.iteration}.pt"
        try:
            with open(self.metadata_path) as f:
                self.metadata: dict[str, Any] = json.load(f)
        except FileNotFoundError:
            self.metadata = {}
        if verbose:
            print(f"Trial loaded from \033[4m{self.checkpoint_path}\033[0m.")

    def load_checkpoint(self, map_location: str | torch.device | None = None):
        return torch.load(self.checkpoint_path, map_location=map_location)

    @classmethod
    def _search_ckpt(cls, directory: Path) -> list[int]:
        return sorted(i for i in map(cls._get_ckpt_iteration, directory.iterdir()) if i is not None)

    @classmethod
    def _is_checkpoint_file(cls, filename: Path) -> bool:
        return filename.is_file() and _CKPT_FILENAME.fullmatch(filename.name) is not None

    @classmethod
    def _get_ckpt_iteration(cls, filename: Path) -> int | None:
        match = _CKPT_FILENAME.fullmatch(filename.name)
        return None if match is None else int(match.group(1))
