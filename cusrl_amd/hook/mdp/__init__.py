from cusrl_amd.hook.mdp.environment_spec import DynamicEnvironmentSpecOverride, EnvironmentSpecOverride
from cusrl_amd.hook.mdp.observation import ObservationNanToNum, ObservationNormalization
from cusrl_amd.hook.mdp.reward import RewardNormalization, RewardShaping

__all__ = [
    "DynamicEnvironmentSpecOverride",
    "EnvironmentSpecOverride",
    "ObservationNanToNum",
    "ObservationNormalization",
    "RewardNormalization",
    "RewardShaping",
]
