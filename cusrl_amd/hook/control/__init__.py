from cusrl_amd.hook.control.condition import ConditionalObjectiveActivation, EpochIndexCondition
from cusrl_amd.hook.control.empty_cuda_cache import EmptyCudaCache
from cusrl_amd.hook.control.initialization import ModuleInitialization
from cusrl_amd.hook.control.optimization_stage import OptimizationStage
from cusrl_amd.hook.control.schedule import HookActivationSchedule, HookParameterSchedule

__all__ = [
    "ConditionalObjectiveActivation",
    "EmptyCudaCache",
    "EpochIndexCondition",
    "HookActivationSchedule",
    "HookParameterSchedule",
    "ModuleInitialization",
    "OptimizationStage",
]
