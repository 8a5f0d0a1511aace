"""Environments that ship with the package: the classic-control tasks as HIP kernels (``classic_control.py``)."""

from cusrl_amd.environment.classic_control import (
    Acrobot, CartPole, ClassicControlEnvironment, MountainCar, MountainCarContinuous, Pendulum, make,
)

__all__ = ["Acrobot", "CartPole", "ClassicControlEnvironment", "MountainCar", "MountainCarContinuous", "Pendulum", "make"]
