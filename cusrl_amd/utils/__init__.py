from cusrl_amd.utils import distributed, scheduler
from cusrl_amd.utils.config import CONFIG, configure_distributed, device, is_autocast_available
from cusrl_amd.utils.distributed import is_main_process
from cusrl_amd.utils.metrics import Metrics
from cusrl_amd.utils.misc import get_first, set_global_seed, to_numpy
from cusrl_amd.utils.scheduler import (
    CosineAnnealingScheduler,
    LessThan,
    NotLessThan,
    PiecewiseLinearScheduler,
    StepScheduler,
    TanhScheduler,
)
from cusrl_amd.utils.timing import Rate, Timer

__all__ = [
    "CONFIG",
    "CosineAnnealingScheduler",
    "LessThan",
    "Metrics",
    "NotLessThan",
    "PiecewiseLinearScheduler",
    "Rate",
    "StepScheduler",
    "TanhScheduler",
    "Timer",
    "configure_distributed",
    "device",
    "distributed",
    "get_first",
    "is_autocast_available",
    "is_main_process",
    "scheduler",
    "set_global_seed",
    "to_numpy",
]
