"""Environments that ship with the package: the classic-control tasks as HIP kernels (``classic_control.py``)."""

from cusrl_amd.environment.classic_control import CartPole, ClassicControlEnvironment, MountainCar, Pendulum, make

__all__ = ["CartPole", "ClassicControlEnvironment", "MountainCar", "Pendulum", "make"]
