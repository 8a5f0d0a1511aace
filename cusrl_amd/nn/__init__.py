from cusrl_amd.nn.actor import Actor, Value
from cusrl_amd.nn.activation import GeGlu, SwiGlu
from cusrl_amd.nn.cnn import Cnn, CnnFactory
from cusrl_amd.nn.causal_attn import CausalMultiheadSelfAttention, CausalTransformerEncoderLayer, compute_segment_ids, get_alibi_slopes
from cusrl_amd.nn.bijector import (
    Bijector, ExponentialBijector, IdentityBijector, SigmoidBijector, SoftplusBijector, make_bijector,
)
from cusrl_amd.nn.attention import MultiheadAttention, MultiheadCrossAttention, MultiheadSelfAttention, make_norm
from cusrl_amd.nn.distribution import AdaptiveNormalDist, Distribution, NormalDist, OneHotCategoricalDist
from cusrl_amd.nn.encoding import RotaryEmbedding
from cusrl_amd.nn.encoding2d import LearnablePositionalEncoding2D, SinusoidalPositionalEncoding2D
from cusrl_amd.nn.deployed import DeployedPolicy
from cusrl_amd.nn.expert import ExpertPolicy
from cusrl_amd.nn.feedforward import FeedForward
from cusrl_amd.nn.gate import (
    Gate, GruGate, HighwayGate, InputGate, OutputGate, PassthroughGate, ResidualGate, SigmoidTanhGate, gate_map, get_gate_cls,
)
from cusrl_amd.nn.inference import InferenceWrapper
from cusrl_amd.nn.loss import L2RegularizationLoss, NormalNllLoss
from cusrl_amd.nn.module import LinearFp32, Mlp, Module, ModuleFactory
from cusrl_amd.nn.normalization import Denormalization, DenormalizationFactory, Normalization, NormalizationFactory
from cusrl_amd.nn.rms import RunningMeanStd
from cusrl_amd.nn.rnn import Gru, Lstm, Rnn
from cusrl_amd.nn.separable_conv import SeparableConv2d
from cusrl_amd.nn.sequential import Sequential, SequentialFactory
from cusrl_amd.nn.simba import Simba, SimbaBlock, SimbaFactory
from cusrl_amd.nn.stacker import ObservationStacker
from cusrl_amd.nn.stub import Identity, StubModule
from cusrl_amd.nn.transformer import TransformerDecoderLayer, TransformerEncoderLayer

__all__ = [
    "Actor",
    "AdaptiveNormalDist",
    "Denormalization",
    "DenormalizationFactory",
    "Distribution",
    "GradientPenaltyLoss",
    "L2RegularizationLoss",
    "LinearFp32",
    "Mlp",
    "Module",
    "ModuleFactory",
    "NormalDist",
    "NormalNllLoss",
    "OneHotCategoricalDist",
    "Gru",
    "Lstm",
    "Normalization",
    "NormalizationFactory",
    "Rnn",
    "RunningMeanStd",
    "Sequential",
    "SequentialFactory",
    "Simba",
    "SimbaBlock",
    "SimbaFactory",
    "Value",
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
    "gate_map",
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
    "Bijector",
    "ExponentialBijector",
    "IdentityBijector",
    "SigmoidBijector",
    "SoftplusBijector",
    "make_bijector",
    "DeployedPolicy",
    "ExpertPolicy",
    "Identity",
    "InferenceWrapper",
    "ObservationStacker",
    "StubModule",
]


def __getattr__(name):
    # GradientPenaltyLoss stays beside its user in hook/auxiliary/amp.py, which itself imports this package: looked up on first
    # use instead of at import
    if name == "GradientPenaltyLoss":
        from cusrl_amd.hook.auxiliary.amp import GradientPenaltyLoss

        return GradientPenaltyLoss
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
