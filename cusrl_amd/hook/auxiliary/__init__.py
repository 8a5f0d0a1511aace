from cusrl_amd.hook.auxiliary.amp import AdversarialMotionPrior
from cusrl_amd.hook.auxiliary.rnd import RandomNetworkDistillation
from cusrl_amd.hook.auxiliary.symmetry import (
    MirrorDef,
    MirrorSymmetryLoss,
    SymmetricDataAugmentation,
    TransitionMirroring,
)

__all__ = [
    "AdversarialMotionPrior",
    "MirrorDef",
    "MirrorSymmetryLoss",
    "RandomNetworkDistillation",
    "SymmetricDataAugmentation",
    "TransitionMirroring",
]
