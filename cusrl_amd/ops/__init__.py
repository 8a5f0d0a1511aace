"""Tensor-level entry points of the HIP hot path, one module per kernel family (grouped as ``cusrl_amd/csrc/*.hip`` is).

Every function takes torch tensors that already live in HBM, passes ``data_ptr()`` + sizes + torch's
current ``hipStream_t`` through the C ABI (``include/cusrl_hip.h``) and returns torch tensors it allocated
with torch's caching allocator.  PyTorch is plumbing here (memory, streams); the arithmetic is in
``cusrl_amd/csrc/*.hip``.  Non-device tensors are rejected — there is deliberately no CPU path.

Callers use ``from cusrl_amd import ops`` and ``ops.<name>(...)``: every entry point is re-exported here.
"""

from __future__ import annotations

import os  # (`os`, `Sequence` and `torch` were reachable as attributes of the one-file module: kept so)
from collections.abc import Sequence

import torch

from cusrl_amd import _native
from cusrl_amd._native import Field, MirrorField, PackedField, check
from cusrl_amd.ops._common import (
    LaunchObserver, _checked, _f32, _flag, _modified_in_place, _observed, _ptr, _raw_stream, _row_bytes, _stream, require_device,
    set_launch_observer,
)
from cusrl_amd.ops.advantage import (
    adv_stats_finalize, col_stats, gae, merge_mean_var, next_value, normalize_, normalize_from_gathered_, normalize_from_partials_,
    packed_mean_var,
)
from cusrl_amd.ops.affine import ColumnAffine, column_affine, column_affine_supported
from cusrl_amd.ops.attention import Rope, Sdpa, rope, rope_supported, sdpa, sdpa_backward, sdpa_supported
from cusrl_amd.ops.band_attention import BandSdpa, band_mask, band_sdpa, band_sdpa_backward, band_sdpa_supported
from cusrl_amd.ops.bias_act import bias_act, bias_act_supported
from cusrl_amd.ops.bijector import BijectorFunction, bijector_supported, sigmoid_bijector, softplus_bijector
from cusrl_amd.ops.auxiliary import (
    accumulate_scalars_, action_smoothness_fwd_bwd, amp_prepare, amp_prepare_supported, amp_style_reward_, amp_style_reward_mean_, bce_pair_fwd_bwd,
    column_mse_fwd_bwd, column_table, masked_col_stats, mse_loss_fwd_bwd, nan_to_num_, normal_nll_bound, normal_nll_fwd_bwd,
    resolve_columns, reward_shaping_, rms_merge_, rms_normalize, rnd_reward_, sumsq_fwd_bwd,
)
from cusrl_amd.ops.buffer import (
    HostCounter, RecordPack, _row_elems, assign_rows, buffer_push, compact_flags, gather_rows, gather_rows_packed, make_push_table,
    push_table, scatter_rows, splice_rows, window_indices,
)
from cusrl_amd.ops.conv import (
    DepthwiseConv2d, depthwise_conv2d, dwconv2d_backward_input, dwconv2d_backward_params, dwconv2d_supported,
)
from cusrl_amd.ops.deploy import deploy_epilogue_, deploy_epilogue_cpu_, deploy_prologue, deploy_prologue_cpu, deploy_supported
from cusrl_amd.ops.environment import (
    CLASSIC_TASKS, ClassicTask, classic_reset, classic_reset_cpu, classic_step, classic_step_cpu,
)
from cusrl_amd.ops.frame_stack import (
    frame_stack_columns, frame_stack_padding, frame_stack_push, frame_stack_push_cpu, frame_stack_reset, frame_stack_reset_cpu,
    frame_stack_supported,
)
from cusrl_amd.ops.gate import GateCombine, Glu, gate_backward, gate_combine, gate_supported, glu, glu_backward, glu_supported
from cusrl_amd.ops.gradient import (
    DeferredColumns, adam_norm_workspace, adam_step, adam_step_normed, adam_step_window, assemble_gradients, clip_grad_norm_,
    grad_sumsq, sum_slabs,
)
from cusrl_amd.ops.graph import graph_census, graph_replace_memsets
from cusrl_amd.ops.layer_norm import AddLayerNorm, add_layer_norm, add_layer_norm_bwd, add_layer_norm_fwd, add_layer_norm_supported
from cusrl_amd.ops.loss import (
    LOSS_DEFER, DeferredLoss, _optional_rows, categorical_policy_stats, categorical_terms_bwd, categorical_terms_fwd, policy_stats,
    policy_terms_bwd, policy_terms_fwd, ppo_loss_accepts_std_vector, ppo_loss_categorical_fwd_bwd, ppo_loss_fwd_bwd,
    value_loss_fwd_bwd,
)
from cusrl_amd.ops.mlp import (
    _HEAD_PAD, input_layer_backward, input_layer_supported, mlp2_forward, mlp2_forward_supported, narrow_linear_backward,
    narrow_linear_forward, narrow_linear_forward_supported, narrow_linear_supported, relu_backward_bias,
)
from cusrl_amd.ops.recurrent import (
    gru_bias_partial_rows, gru_bias_partials_supported, gru_gates_backward, gru_gates_forward, lstm_gates_backward,
    lstm_gates_forward, rnn_cell_backward, rnn_cell_forward,
)
from cusrl_amd.ops.reward import reward_normalize_, reward_normalize_cpu_
from cusrl_amd.ops.rollout import (
    PendingStepEpilogue, categorical_sample_logp, episode_stats, normal_sample_logp, play_epilogue, play_epilogue_workspace,
    step_epilogue, synthetic_env_step,
)
from cusrl_amd.ops.symmetry import (
    _mirror_table, _rows_2d, mirror_mse_fwd_bwd, mirror_rows, mirror_rows_bwd, symmetric_head_bwd, symmetric_head_fwd,
    symmetric_head_sample, symmetric_head_supported, symmetrize_mean_var_,
)
