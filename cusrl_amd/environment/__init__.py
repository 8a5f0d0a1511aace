"""Environments that ship with the package: the classic-control tasks as HIP kernels (``classic_control.py``) and the
observation-history wrapper that composes with them (``frame_stack.py``)."""

from cusrl_amd.environment.classic_control import (
    Acrobot, CartPole, ClassicControlEnvironment, MountainCar, MountainCarContinuous, Pendulum, make,
)
from cusrl_amd.environment.frame_stack import FrameStack

__all__ = ["Acrobot", "CartPole", "ClassicControlEnvironment", "FrameStack", "MountainCar", "MountainCarContinuous", "Pendulum", "make"]
