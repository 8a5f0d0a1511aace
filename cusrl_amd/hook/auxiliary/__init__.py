from cusrl_amd.hook.auxiliary.amp import AdversarialMotionPrior
from cusrl_amd.hook.auxiliary.distillation import PolicyDistillation, PolicyDistillationLoss
from cusrl_amd.hook.auxiliary.estimation import StateEstimation
from cusrl_amd.hook.auxiliary.representation import NextStatePrediction, ReturnPrediction, StatePrediction
from cusrl_amd.hook.auxiliary.rnd import RandomNetworkDistillation
from cusrl_amd.hook.auxiliary.smoothness import ActionSmoothnessLoss
from cusrl_amd.hook.auxiliary.symmetry import (
    MirrorDef,
    MirrorSymmetryLoss,
    SymmetricActor,
    SymmetricActorFactory,
    SymmetricArchitecture,
    SymmetricDataAugmentation,
    TransitionMirroring,
)

__all__ = [
    "ActionSmoothnessLoss",
    "AdversarialMotionPrior",
    "MirrorDef",
    "MirrorSymmetryLoss",
    "NextStatePrediction",
    "PolicyDistillation",
    "PolicyDistillationLoss",
    "RandomNetworkDistillation",
    "ReturnPrediction",
    "StateEstimation",
    "StatePrediction",
    "SymmetricActor",
    "SymmetricActorFactory",
    "SymmetricArchitecture",
    "SymmetricDataAugmentation",
    "TransitionMirroring",
]
