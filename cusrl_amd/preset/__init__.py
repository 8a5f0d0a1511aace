from cusrl_amd.preset.distillation import DistillationAgentFactory, distillation_hook_suite
from cusrl_amd.preset.ppo import AdamFactory, AmpAgentFactory, PpoAgentFactory, RecurrentPpoAgentFactory, ppo_hook_suite

__all__ = ["AdamFactory", "AmpAgentFactory", "DistillationAgentFactory", "PpoAgentFactory", "RecurrentPpoAgentFactory",
           "distillation_hook_suite", "ppo_hook_suite"]
