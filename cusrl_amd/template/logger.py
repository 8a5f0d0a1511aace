"""The run directory a ``Trainer`` logs and checkpoints into (counterpart of cusrl/template/logger.py:19-165).

``Logger(log_dir, name)`` lays out ``log_dir/[timestamp_]name/{info,ckpt}`` and points ``log_dir/latest`` at it (rank 0 only; every
rank learns rank 0's directory), averages logged data over ``interval`` calls, writes ``ckpt/ckpt_{i}.pt`` and text files under
``info/``.  What is done with the logged numbers is a subclass's ``_log_impl``; the TensorBoard / W&B / SwanLab subclasses of the
reference are not part of this package, so ``make_logger_factory`` knows ``None`` / ``"none"`` and whatever subclasses the caller
has defined."""

from __future__ import annotations

import os
from collections.abc import Callable
from datetime import datetime
from pathlib import Path
from typing import TypeAlias

import torch

from cusrl_amd.utils import distributed, switches

__all__ = ["Logger", "LoggerFactory", "LoggerFactoryLike", "make_logger_factory"]


class LoggerFactory:
    def __init__(self, log_dir: str | os.PathLike, name: str | None = "", interval: int = 1, add_datetime_prefix: bool = True):
        self.log_dir = log_dir
        self.name = name
        self.interval = interval
        self.add_datetime_prefix = add_datetime_prefix

    def __call__(self) -> "Logger":
        return Logger(log_dir=self.log_dir, name=self.name, interval=self.interval, add_datetime_prefix=self.add_datetime_prefix)


LoggerFactoryLike: TypeAlias = Callable[[], "Logger"]


class Logger:
    Factory = LoggerFactory

    def __init__(self, log_dir: str | os.PathLike, name: str | None = "", interval: int = 1, add_datetime_prefix: bool = True):
        self.log_dir = Path(log_dir).absolute()
        self.name = name
        if self.name is not None:
            if "/" in self.name or "\\" in self.name:
                raise ValueError("'name' must not contain '/' or '\\' characters")
            if add_datetime_prefix:
                timestamp = datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
                self.name = f"{timestamp}_{self.name}" if self.name else timestamp
            self.log_dir /= self.name
        self.log_dir = Path(distributed.gather_obj(str(self.log_dir))[0])
        switches.publish("TRIAL_LOG_DIR", str(self.log_dir))
        self.info_dir = self.log_dir / "info"
        self.ckpt_dir = self.log_dir / "ckpt"

        if distributed.is_main_process():
            self.log_dir.mkdir(parents=True, exist_ok=True)
            if self.name is not None:
                symlink_path = self.log_dir.parent / "latest"
                symlink_path.unlink(missing_ok=True)
                symlink_path.symlink_to(self.log_dir.name, target_is_directory=True)
            self.info_dir.mkdir(exist_ok=True)
            self.ckpt_dir.mkdir(exist_ok=True)

        self.interval = interval
        self.data_list: list[dict[str, float]] = []

    def log(self, data: dict[str, float], iteration: int):
        if self.interval > 1:
            self.data_list.append(data)
            if len(self.data_list) < self.interval:
                return
            data = self._collect_data()
            self.data_list.clear()
        self._log_impl(data, iteration)

    def save_checkpoint(self, state_dict, iteration: int):
        torch.save(state_dict, self.ckpt_dir / f"ckpt_{iteration}.pt")

    def save_info(self, info_str: str, filename: str):
        path = self.info_dir / filename
        path.parent.mkdir(parents=True, exist_ok=True)
        with open(path, "w") as f:
            f.write(info_str)

    def _collect_data(self):
        collection: dict[str, list[float]] = {}
        for data in self.data_list:
            for key, val in data.items():
                collection.setdefault(key, []).append(val)
        return {key: sum(val) / len(val) for key, val in collection.items()}

    def _log_impl(self, data: dict[str, float], iteration: int):
        pass


def make_logger_factory(logger_type: str | None = None, log_dir: str | os.PathLike | None = None, name: str | None = "",
                        interval: int = 1, add_datetime_prefix: bool = True, **kwargs) -> LoggerFactoryLike | None:
    if log_dir is None:
        return None
    if logger_type is None or logger_type.lower() == "none":
        logger_cls = Logger
    else:
        logger_cls = {cls.__name__.lower(): cls for cls in Logger.__subclasses__()}[logger_type.lower()]  # KeyError: unknown type
    return logger_cls.Factory(log_dir=log_dir, name=name, interval=interval, add_datetime_prefix=add_datetime_prefix, **kwargs)
