"""cusrl_amd — MI355X-native vectorised-rollout + PPO-update engine behind the cusrl plugin surface.

``import cusrl_amd as cusrl`` and the `ppo` preset, ``Buffer`` / ``Sampler`` / ``Hook`` / ``Trainer`` read like
chengruiz/cusrl; the per-iteration hot path (buffer append, next_value, GAE, advantage normalisation, minibatch
gather, PPO objective forward+backward) runs as hand-written HIP kernels for gfx950 through ``libcusrl_hip.so``.
"""

from cusrl_amd import environment, hook, nn, preset, sampler, template, testing, utils
from cusrl_amd.hook import NextStatePrediction, PolicyDistillation, PolicyDistillationLoss, ReturnPrediction, StateEstimation, StatePrediction
from cusrl_amd.nn import (
    Actor, AdaptiveNormalDist, Denormalization, DenormalizationFactory, Distribution, GradientPenaltyLoss, Gru, L2RegularizationLoss,
    LinearFp32, Lstm, Mlp, Module, ModuleFactory, NormalDist, NormalNllLoss, Normalization, NormalizationFactory,
    OneHotCategoricalDist, Rnn, RunningMeanStd, Sequential, SequentialFactory, Simba, SimbaBlock, SimbaFactory, Value,
)
from cusrl_amd.nn import (
    FeedForward, Gate, GeGlu, GruGate, HighwayGate, InputGate, OutputGate, PassthroughGate, ResidualGate, SigmoidTanhGate, SwiGlu,
    get_gate_cls,
)
from cusrl_amd.nn import (
    MultiheadAttention, MultiheadCrossAttention, MultiheadSelfAttention, RotaryEmbedding, TransformerDecoderLayer,
    TransformerEncoderLayer, make_norm,
)
from cusrl_amd.nn import CausalMultiheadSelfAttention, CausalTransformerEncoderLayer, compute_segment_ids, get_alibi_slopes
from cusrl_amd.nn import Cnn, CnnFactory, LearnablePositionalEncoding2D, SeparableConv2d, SinusoidalPositionalEncoding2D
from cusrl_amd.nn import DeployedPolicy, ExpertPolicy, Identity, InferenceWrapper, ObservationStacker, StubModule
from cusrl_amd.environment import FrameStack
from cusrl_amd.sampler import (
    AutoMiniBatchSampler, AutoRandomSampler, MiniBatchSampler, RandomSampler, TemporalMiniBatchSampler, TemporalRandomSampler,
)
from cusrl_amd.template import (
    ActorCritic,
    Agent,
    Buffer,
    Environment,
    EnvironmentSpec,
    Hook,
    Logger,
    LoggerFactory,
    OptimizerFactory,
    Player,
    PlayerHook,
    Sampler,
    Trainer,
    TrainerHook,
    Trial,
    make_logger_factory,
)
from cusrl_amd.utils import CONFIG as config
from cusrl_amd.utils import device, set_global_seed
from cusrl_amd import zoo  # (after everything it registers experiments from)

__version__ = "0.1.0"

__all__ = [
    "Actor",
    "ActorCritic",
    "AdaptiveNormalDist",
    "Agent",
    "AutoMiniBatchSampler",
    "AutoRandomSampler",
    "Buffer",
    "Denormalization",
    "DenormalizationFactory",
    "Distribution",
    "Environment",
    "EnvironmentSpec",
    "GradientPenaltyLoss",
    "Gru",
    "Hook",
    "L2RegularizationLoss",
    "LinearFp32",
    "Lstm",
    "MiniBatchSampler",
    "Mlp",
    "Module",
    "ModuleFactory",
    "NextStatePrediction",
    "NormalDist",
    "NormalNllLoss",
    "Normalization",
    "NormalizationFactory",
    "OneHotCategoricalDist",
    "OptimizerFactory",
    "PolicyDistillationLoss",
    "RandomSampler",
    "ReturnPrediction",
    "Rnn",
    "RunningMeanStd",
    "Sampler",
    "Sequential",
    "SequentialFactory",
    "Simba",
    "SimbaBlock",
    "SimbaFactory",
    "StateEstimation",
    "StatePrediction",
    "TemporalMiniBatchSampler",
    "TemporalRandomSampler",
    "Trainer",
    "TrainerHook",
    "Value",
    "config",
    "device",
    "hook",
    "environment",
    "nn",
    "preset",
    "sampler",
    "set_global_seed",
    "template",
    "testing",
    "utils",
    "FeedForward",
    "Gate",
    "GeGlu",
    "GruGate",
    "HighwayGate",
    "InputGate",
    "OutputGate",
    "PassthroughGate",
    "ResidualGate",
    "SigmoidTanhGate",
    "SwiGlu",
    "get_gate_cls",
    "MultiheadAttention",
    "MultiheadCrossAttention",
    "MultiheadSelfAttention",
    "RotaryEmbedding",
    "TransformerDecoderLayer",
    "TransformerEncoderLayer",
    "make_norm",
    "CausalMultiheadSelfAttention",
    "CausalTransformerEncoderLayer",
    "compute_segment_ids",
    "get_alibi_slopes",
    "Cnn",
    "CnnFactory",
    "LearnablePositionalEncoding2D",
    "SeparableConv2d",
    "SinusoidalPositionalEncoding2D",
    "DeployedPolicy",
    "ExpertPolicy",
    "Identity",
    "PolicyDistillation",
    "StubModule",
    "InferenceWrapper",
    "Logger",
    "LoggerFactory",
    "Player",
    "PlayerHook",
    "Trial",
    "make_logger_factory",
    "zoo",
    "FrameStack",
    "ObservationStacker",
]
