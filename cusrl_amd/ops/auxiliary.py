"""Running statistics and the auxiliary hooks' kernels: RND / AMP rewards, reward shaping, small losses, scalar
accumulation (``csrc/normalization.hip``, ``aux_hooks.hip``)."""

from __future__ import annotations

import ctypes
import math
from collections.abc import Sequence

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _f32, _flag, _loss_outputs, _modified_in_place, _ptr, _stream, require_device


def masked_col_stats(x: torch.Tensor, mask: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``mean_var_count`` (population variance) of the rows of ``x [rows, C]`` whose ``mask`` byte is set
    (cusrl/nn/utils/normalization.py:15-50 after the ``observation[indices]`` select of observation.py:206-208);
    the count stays on the device (double[1]) — no host synchronisation."""
    x = _f32(x, "input")
    C = x.shape[-1]
    rows = x.numel() // C
    if mask is not None:
        mask = _flag(mask, "mask")
        if mask.numel() != rows:
            raise ValueError("masked_col_stats: mask must have one entry per row")
    lib = _native.lib()
    dev = x.device
    partials = torch.empty((max(int(lib.cusrl_masked_stats_num_partials(rows, C)), 1), C + 1, 2), dtype=torch.float64, device=dev)
    mean, var = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.float64, device=dev)
    _checked.cusrl_masked_col_stats(x.data_ptr(), _ptr(mask), rows, C, partials.data_ptr(), mean.data_ptr(), var.data_ptr(),
            count.data_ptr(), _stream())
    return mean, var, count


def rms_merge_(mean, var, std, count, batch_mean, batch_var, batch_count, eps: float, max_count: float | None) -> None:
    """In-place Chan merge of batch statistics into running statistics (normalization.py:80-93, rms.py:163-167)."""
    _checked.cusrl_rms_merge(
        _f32(mean, "mean").data_ptr(), _f32(var, "var").data_ptr(), _f32(std, "std").data_ptr(), count.data_ptr(),
        _f32(batch_mean, "batch_mean").data_ptr(), _f32(batch_var, "batch_var").data_ptr(), batch_count.data_ptr(),
        float(eps), -1.0 if max_count is None else float(max_count), mean.numel(), _stream(),
    )


def rms_normalize(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, clamp: float | None) -> torch.Tensor:
    """``((x - mean) / std).clamp(-clamp, clamp)`` as one launch (rms.py:198-203)."""
    x = _f32(x, "input")
    C = x.shape[-1]
    out = torch.empty_like(x)
    _checked.cusrl_rms_normalize(x.data_ptr(), _f32(mean, "mean").data_ptr(), _f32(std, "std").data_ptr(),
            -1.0 if clamp is None else float(clamp),
            out.data_ptr(), x.numel() // C, C, _stream())
    return out


def rnd_reward_(reward: torch.Tensor, target: torch.Tensor, prediction: torch.Tensor, scale: float) -> torch.Tensor:
    """``reward += scale * (target - prediction).square().mean(-1, keepdim=True)`` in place, one launch; returns the
    added bonus (cusrl/hook/auxiliary/rnd.py:71-74)."""
    target, prediction = _f32(target, "target"), _f32(prediction, "prediction")
    require_device(reward, "reward")
    if reward.dtype != torch.float32 or not reward.is_contiguous() or reward.shape[-1] != 1:
        raise TypeError("rnd_reward_: reward must be a contiguous float32 [..., 1] tensor")
    K = target.shape[-1]
    rows = target.numel() // K
    if reward.numel() != rows or prediction.shape != target.shape:
        raise ValueError("rnd_reward_: shape mismatch")
    bonus = torch.empty_like(reward)
    _checked.cusrl_rnd_reward(target.data_ptr(), prediction.data_ptr(), reward.data_ptr(), bonus.data_ptr(), float(scale), rows, K, _stream())
    _modified_in_place(reward)
    return bonus


def amp_style_reward_(reward: torch.Tensor, logit: torch.Tensor, scale: float) -> torch.Tensor:
    """``reward += scale * -log(clamp(1 - sigmoid(logit), 1e-4))`` in place, one launch; returns the bonus
    (cusrl/hook/auxiliary/amp.py:134-136)."""
    logit = _f32(logit, "logit")
    require_device(reward, "reward")
    if reward.dtype != torch.float32 or not reward.is_contiguous() or reward.numel() != logit.numel():
        raise TypeError("amp_style_reward_: reward must be a contiguous float32 tensor matching the logits")
    bonus = torch.empty_like(reward)
    _checked.cusrl_amp_style_reward(logit.data_ptr(), reward.data_ptr(), bonus.data_ptr(), float(scale), logit.numel(), _stream())
    _modified_in_place(reward)
    return bonus


def amp_style_reward_mean_(reward: torch.Tensor, logit: torch.Tensor, scale: float) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`amp_style_reward_` + the mean of the bonus (what ``agent.record(amp_reward=...)`` reduces) from ONE launch;
    returns ``(bonus, mean[1])``.  Falls back to the two-launch form beyond the single-workgroup size."""
    logit = _f32(logit, "logit")
    require_device(reward, "reward")
    if reward.dtype != torch.float32 or not reward.is_contiguous() or reward.numel() != logit.numel():
        raise TypeError("amp_style_reward_mean_: reward must be a contiguous float32 tensor matching the logits")
    if logit.numel() > (1 << 20):
        bonus = amp_style_reward_(reward, logit, scale)
        return bonus, bonus.mean().reshape(1)
    bonus = torch.empty_like(reward)
    mean = torch.empty(1, dtype=torch.float32, device=reward.device)
    _checked.cusrl_amp_style_reward_mean(logit.data_ptr(), reward.data_ptr(), bonus.data_ptr(), float(scale), logit.numel(),
            mean.data_ptr(), _stream())
    _modified_in_place(reward)
    return bonus, mean


def amp_prepare_supported(rows: int, channels: int) -> bool:
    return 0 < channels <= 128 and 0 < rows * channels <= int(_native.lib().cusrl_amp_prepare_max_elements())


def amp_prepare(rms, *, state=None, next_state=None, columns=None, width: int | None = None, agent_raw=None, dataset=None,
                indices=None, expert_raw=None) -> tuple[torch.Tensor, torch.Tensor]:
    """AMP's ``post_step`` up to the discriminator (amp.py:112-128) as ONE C-ABI call (two launches): assemble ``state[cols] || next_state[cols]``
    (or take ``agent_raw``), fetch ``dataset[indices]`` (or take ``expert_raw``), update ``rms`` (a RunningMeanStd) with the
    agent rows, then the expert rows, normalise both.  ``columns``: int32 device vector of the selected state columns, or
    None with ``width`` = K for the first K columns.  Returns ``(agent_transition, expert_transition)``, ``[N, C]`` each."""
    if agent_raw is not None:
        agent_raw = _f32(agent_raw, "agent_raw")
        N, C = agent_raw.shape
        K = C // 2
    else:
        state, next_state = _f32(state, "state"), _f32(next_state, "next_state")
        if state.dim() != 2 or state.shape != next_state.shape:
            raise ValueError("amp_prepare: state / next_state must be [N, S] tensors of one shape")
        N = state.shape[0]
        K = int(columns.numel()) if columns is not None else int(width)
        C = 2 * K
        if columns is not None and (columns.dtype != torch.int32 or not columns.is_cuda):
            raise TypeError("amp_prepare: 'columns' must be an int32 device vector")
    if expert_raw is not None:
        expert_raw = _f32(expert_raw, "expert_raw")
        if tuple(expert_raw.shape) != (N, C):
            raise ValueError("amp_prepare: expert rows do not match the agent rows")
    else:
        dataset = _f32(dataset, "dataset")
        if indices.dtype != torch.int64 or indices.numel() != N or dataset.shape[-1] != C:
            raise ValueError("amp_prepare: need one int64 dataset index per agent row and rows of the transition's width")
        indices = indices.contiguous()
    dev = rms.mean.device
    agent_out = torch.empty((N, C), dtype=torch.float32, device=dev)
    expert_out = torch.empty((N, C), dtype=torch.float32, device=dev)
    workspace = torch.empty(max(int(_native.lib().cusrl_amp_prepare_workspace(N, C)), 1), dtype=torch.float64, device=dev)
    _checked.cusrl_amp_prepare(
        _ptr(state), _ptr(next_state), 0 if state is None else state.shape[1], _ptr(columns), K, _ptr(agent_raw), _ptr(dataset),
        _ptr(indices), _ptr(expert_raw), N, C, rms.mean.data_ptr(), rms.var.data_ptr(), rms.std.data_ptr(), rms._count.data_ptr(),
        float(rms.epsilon), -1.0 if rms.max_count is None else float(rms.max_count), -1.0 if rms.clamp is None else float(rms.clamp),
        agent_out.data_ptr(), expert_out.data_ptr(), workspace.data_ptr(), _stream(),
    )
    return agent_out, expert_out


def reward_shaping_(reward: torch.Tensor, scale: float, shift: float, lower: float | None, upper: float | None) -> torch.Tensor:
    """``reward.mul_(scale).add_(shift).clamp_(lower, upper)`` (reward.py:43-47) in place, one launch."""
    require_device(reward, "reward")
    if reward.dtype != torch.float32 or not reward.is_contiguous():
        raise TypeError("reward_shaping_: expected a contiguous float32 tensor")
    _checked.cusrl_reward_shaping(reward.data_ptr(), float(scale), float(shift), 0.0 if lower is None else float(lower),
            0.0 if upper is None else float(upper), int(lower is not None), int(upper is not None), reward.numel(), _stream())
    _modified_in_place(reward)
    return reward


def nan_to_num_(a: torch.Tensor, b: torch.Tensor | None = None, *, nan: float = 0.0, posinf: float = 0.0,
                neginf: float = 0.0) -> torch.Tensor:
    """``a.nan_to_num_(nan, posinf, neginf)`` — and the same of ``b`` when given — in place, ONE launch for both
    (observation.py:42-56: the observation and the state of one hook call).  Finite values keep their bit patterns; only the
    16-byte lanes that held a NaN or an infinity are written back.  Returns ``a``."""
    for name, tensor in (("a", a), ("b", b)):
        if tensor is None:
            continue
        require_device(tensor, name)
        if tensor.dtype != torch.float32 or not tensor.is_contiguous():
            raise TypeError(f"nan_to_num_: '{name}' must be a contiguous float32 tensor")
    _checked.cusrl_nan_to_num2(a.data_ptr(), a.numel(), _ptr(b), 0 if b is None else b.numel(), float(nan), float(posinf),
            float(neginf), _stream())
    _modified_in_place(a)
    if b is not None:
        _modified_in_place(b)
    return a


def mse_loss_fwd_bwd(prediction: torch.Tensor, target: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(mean((prediction - target)^2), d loss / d prediction)`` from one pass (+ a one-block finalize)."""
    prediction, target = _f32(prediction, "prediction"), _f32(target, "target")
    if prediction.shape != target.shape or prediction.numel() == 0:
        raise ValueError("mse_loss_fwd_bwd: shapes differ or are empty")
    n = prediction.numel()
    loss, partials = _loss_outputs(prediction.device, _native.lib().cusrl_mse_loss_num_partials(n))
    grad = torch.empty_like(prediction)
    _checked.cusrl_mse_loss_fwd_bwd(prediction.data_ptr(), target.data_ptr(), n, loss.data_ptr(), grad.data_ptr(), partials.data_ptr(), _stream())
    return loss, grad


def resolve_columns(indices, width: int) -> torch.Tensor | None:
    """The columns ``target[..., indices]`` selects of a ``width``-wide target, as a host int32 vector:
    ``torch.arange(width)[indices]`` (a slice, an int list or an index tensor; negative entries resolved), or None for
    ``slice(None)`` — every column in place.  A slice is resolved as Python resolves it, so a negative step (which torch's
    own indexing refuses) selects the columns in descending order."""
    if isinstance(indices, slice):
        if indices == slice(None):
            return None
        resolved = torch.tensor(list(range(int(width))[indices]), dtype=torch.int32)
    else:
        if isinstance(indices, torch.Tensor):
            indices = indices.cpu()
        resolved = torch.arange(int(width))[indices].reshape(-1).to(torch.int32)
    if resolved.numel() == 0:
        raise ValueError(f"{indices!r} selects no column of a {width}-wide target")
    return resolved


def column_table(indices, width: int, device) -> torch.Tensor | None:
    """:func:`resolve_columns` as the int32 device table of ``cusrl_column_mse_fwd_bwd`` (None stays None).  Uploaded here —
    call it outside any capture."""
    resolved = resolve_columns(indices, width)
    if resolved is None:
        return None
    table = resolved.to(device)
    table._cusrl_column_range = (int(resolved.min()), int(resolved.max()))  # what the binding validates against the pitch
    return table


def _target_rows(target: torch.Tensor) -> tuple[torch.Tensor, int]:
    """``(tensor, row pitch in elements)`` of a ``[..., W]`` target whose rows lie one pitch apart (a contiguous tensor, or a
    row / column view of one with last-dim stride 1); anything else is staged contiguously."""
    W = target.shape[-1]
    lead = [(size, stride) for size, stride in zip(target.shape[:-1], target.stride()[:-1]) if size != 1]
    pitch = lead[-1][1] if lead else W
    uniform = target.stride(-1) == 1 and pitch >= W and all(
        outer[1] == inner[0] * inner[1] for outer, inner in zip(lead[:-1], lead[1:]))
    if not uniform:
        target, pitch = target.contiguous(), W
    return target, pitch


def column_mse_fwd_bwd(prediction: torch.Tensor, target: torch.Tensor, columns: torch.Tensor | None,
                       weight: float) -> tuple[torch.Tensor, torch.Tensor]:
    """``(weight * mean((prediction - target[..., columns])^2), d loss / d prediction)`` from one pass (+ a one-block finalize
    beyond one block).  ``prediction [..., K]``; ``target [..., W]`` with the same leading shape is read IN PLACE (a buffer
    leaf, or a view whose last-dim stride is 1); ``columns``: a :func:`column_table` (or any int32 device vector of K entries),
    None for the first K columns."""
    prediction = _f32(prediction, "prediction")
    require_device(target, "target")
    if target.dtype != torch.float32:
        raise TypeError(f"'target' must be float32, got {target.dtype}")
    K, W = prediction.shape[-1], target.shape[-1]
    if prediction.numel() == 0 or prediction.shape[:-1] != target.shape[:-1]:
        raise ValueError(f"column_mse_fwd_bwd: prediction {tuple(prediction.shape)} and target {tuple(target.shape)} differ in "
                         "their leading shape or are empty")
    if columns is None:
        if K > W:
            raise ValueError(f"column_mse_fwd_bwd: a {K}-wide prediction against a {W}-wide target")
    else:
        if columns.dtype != torch.int32 or not columns.is_cuda or columns.dim() != 1 or not columns.is_contiguous():
            raise TypeError("column_mse_fwd_bwd: 'columns' must be a contiguous int32 device vector")
        if columns.numel() != K:
            raise ValueError(f"column_mse_fwd_bwd: {columns.numel()} columns for a {K}-wide prediction")
        low, high = getattr(columns, "_cusrl_column_range", None) or (int(columns.min()), int(columns.max()))
        if low < 0 or high >= W:
            raise IndexError(f"column_mse_fwd_bwd: columns {low}..{high} out of range for a {W}-wide target")
    target, pitch = _target_rows(target)
    rows = prediction.numel() // K
    loss, partials = _loss_outputs(prediction.device, _native.lib().cusrl_column_mse_num_partials(rows, K))
    grad = torch.empty_like(prediction)
    _checked.cusrl_column_mse_fwd_bwd(prediction.data_ptr(), target.data_ptr(), pitch, _ptr(columns), rows, K, float(weight),
            loss.data_ptr(), grad.data_ptr(), partials.data_ptr(), _stream())
    return loss, grad


NORMAL_NLL_MODES = {"log_var": 0, "log_std": 1, "var": 2, "std": 3}
_REDUCTIONS = {"mean": 1, "sum": 2}


def normal_nll_bound(mode: str, eps: float) -> float:
    """The clamp bound of ``NormalNllLoss`` in the variance parameter's own domain (cusrl/nn/layer/loss.py:116-129), in double."""
    eps = float(eps)
    return {"log_var": math.log(eps), "log_std": math.log(eps) / 2, "var": eps, "std": math.sqrt(eps)}[mode]


def normal_nll_fwd_bwd(mean: torch.Tensor, dist: torch.Tensor | None, target: torch.Tensor, mode: str, full: bool, eps: float,
                       reduction: str) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(NormalNllLoss(mode, full, eps, reduction)(input, target), d loss / d mean, d loss / d dist)`` from one pass (+ a
    one-block finalize beyond one block).  ``mean`` / ``dist [..., K]``: the tuple input; ``dist`` None: ``mean`` is the chunked
    ``[..., 2K]`` input, read in place as its two halves, and the two gradients are the halves of ONE ``[..., 2K]`` tensor
    (``d_mean._base``) — no ``cat``, no zero-fill.  ``target [..., K]`` with the same leading shape is read in place where its rows
    lie one pitch apart (a column view of a wider leaf), staged contiguously otherwise."""
    if mode not in NORMAL_NLL_MODES or reduction not in _REDUCTIONS:
        raise ValueError(f"normal_nll_fwd_bwd: mode {mode!r} / reduction {reduction!r} (the kernel reduces by 'mean' or 'sum')")
    mean = _f32(mean, "mean" if dist is not None else "input")
    require_device(target, "target")
    if target.dtype != torch.float32:
        raise TypeError(f"'target' must be float32, got {target.dtype}")
    if dist is None:
        if mean.dim() < 1 or mean.shape[-1] % 2:
            raise ValueError(f"normal_nll_fwd_bwd: a chunked input {tuple(mean.shape)} needs an even last dimension")
        K = mean.shape[-1] // 2
        shape, pitch = (*mean.shape[:-1], K), 2 * K
        grad = torch.empty_like(mean)
        d_mean, d_dist = grad[..., :K], grad[..., K:]
        dist_ptr = mean.data_ptr() + 4 * K
    else:
        dist = _f32(dist, "dist")
        if mean.dim() < 1 or dist.shape != mean.shape:
            raise ValueError(f"normal_nll_fwd_bwd: mean {tuple(mean.shape)} and dist {tuple(dist.shape)} differ in shape")
        K = mean.shape[-1]
        shape, pitch = tuple(mean.shape), K
        d_mean, d_dist = torch.empty_like(mean), torch.empty_like(dist)
        dist_ptr = dist.data_ptr()
    if mean.numel() == 0 or tuple(target.shape) != tuple(shape):
        raise ValueError(f"normal_nll_fwd_bwd: input halves {tuple(shape)} and target {tuple(target.shape)} differ in shape or "
                         "are empty")
    target, target_pitch = _target_rows(target)
    rows = d_mean.numel() // K
    loss, partials = _loss_outputs(mean.device, _native.lib().cusrl_normal_nll_num_partials(rows, K))
    _checked.cusrl_normal_nll_fwd_bwd(mean.data_ptr(), pitch, dist_ptr, pitch, target.data_ptr(), target_pitch, rows, K,
            NORMAL_NLL_MODES[mode], int(bool(full)), normal_nll_bound(mode, eps), _REDUCTIONS[reduction], loss.data_ptr(),
            d_mean.data_ptr(), d_dist.data_ptr(), pitch, partials.data_ptr(), _stream())
    return loss, d_mean, d_dist


def action_smoothness_fwd_bwd(mean: torch.Tensor, done: torch.Tensor, w1: torch.Tensor | None,
                              w2: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ActionSmoothnessLoss`` (cusrl/hook/auxiliary/smoothness.py:59-102) of ``mean [T, B, A]`` cut at ``done [T, B, 1]``, from
    ONE C-ABI call: ``(losses fp32[2], counts int64[2], d_mean)``.  ``w1`` / ``w2``: fp32 device ``[A]`` weight vectors of the
    first- / second-order term, None: that term is not evaluated (its loss slot is 0).  ``d_mean [planes, T, B, A]`` holds one
    gradient plane per given weight, the first order's first — the terms' gradients stay apart.  ``counts``: the numbers of valid
    pairs and triples, left on the device.  A non-contiguous ``mean`` is staged contiguously."""
    mean, done = _f32(mean, "mean"), _flag(done, "done")
    if mean.dim() != 3:
        raise ValueError(f"action_smoothness_fwd_bwd: mean must be [T, B, A], got {tuple(mean.shape)}")
    T, B, A = mean.shape
    if T < 3 or B == 0 or A == 0:
        raise ValueError(f"action_smoothness_fwd_bwd: mean {tuple(mean.shape)} needs at least 3 time steps and no empty dimension")
    if done.numel() != T * B or tuple(done.shape[:2]) != (T, B):
        raise ValueError(f"action_smoothness_fwd_bwd: done {tuple(done.shape)} is not [T, B, 1] of mean {tuple(mean.shape)}")
    if w1 is None and w2 is None:
        raise ValueError("action_smoothness_fwd_bwd: neither term has a weight")
    for name, weight in (("w1", w1), ("w2", w2)):
        if weight is None:
            continue
        require_device(weight, name)
        if weight.dtype != torch.float32 or not weight.is_contiguous() or tuple(weight.shape) != (A,):
            raise TypeError(f"action_smoothness_fwd_bwd: '{name}' must be a contiguous float32 [{A}] device vector")
    words = int(_native.lib().cusrl_action_smoothness_workspace(T, B, A))
    if words == 0:
        raise ValueError(f"action_smoothness_fwd_bwd: mean {tuple(mean.shape)} is beyond a 32-bit element index")
    dev = mean.device
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    d_mean = torch.empty(((w1 is not None) + (w2 is not None), T, B, A), dtype=torch.float32, device=dev)
    workspace = torch.empty(words, dtype=torch.float64, device=dev)
    _checked.cusrl_action_smoothness_fwd_bwd(mean.data_ptr(), done.data_ptr(), _ptr(w1), _ptr(w2), T, B, A, losses.data_ptr(),
            counts.data_ptr(), d_mean.data_ptr(), workspace.data_ptr(), _stream())
    return losses, counts, d_mean


def sumsq_fwd_bwd(x: torch.Tensor, loss_scale: float, grad_scale: float) -> tuple[torch.Tensor, torch.Tensor]:
    """``(loss_scale * sum(x^2), grad_scale * x)`` from one pass (AMP's gradient penalty and what it sends back)."""
    x = _f32(x, "x")
    n = x.numel()
    loss, partials = _loss_outputs(x.device, _native.lib().cusrl_mse_loss_num_partials(n))
    grad = torch.empty_like(x)
    _checked.cusrl_sumsq_fwd_bwd(x.data_ptr(), n, float(loss_scale), float(grad_scale), loss.data_ptr(), grad.data_ptr(),
            partials.data_ptr(), _stream())
    return loss, grad


def bce_pair_fwd_bwd(logit: torch.Tensor, weight: float) -> tuple[torch.Tensor, torch.Tensor]:
    """Discrimination loss of a joint ``[2N, 1]`` logit batch (agent rows first: target 0, expert rows: target 1) times
    ``weight``, and its gradient wrt the logits — one launch."""
    logit = _f32(logit, "logit")
    if logit.numel() % 2:
        raise ValueError("bce_pair_fwd_bwd: the joint batch holds as many expert as agent rows")
    loss, _ = _loss_outputs(logit.device)
    grad = torch.empty_like(logit)
    _checked.cusrl_bce_pair_fwd_bwd(logit.data_ptr(), logit.numel() // 2, float(weight), loss.data_ptr(), grad.data_ptr(), _stream())
    return loss, grad


def accumulate_scalars_(accumulator: torch.Tensor, values: Sequence[torch.Tensor]) -> None:
    """``accumulator[i] += values[i]`` for 0-d fp32 device tensors — ONE launch per 32 values (pointer table by value)."""
    if accumulator.dtype != torch.float32 or not accumulator.is_contiguous() or accumulator.numel() < len(values):
        raise ValueError("accumulate_scalars_: need a contiguous float32 accumulator with one slot per value")
    staged = [v if v.dtype == torch.float32 else v.float() for v in values]
    for start in range(0, len(staged), 32):
        chunk = staged[start:start + 32]
        table = (ctypes.c_void_p * len(chunk))(*[require_device(v, "value").data_ptr() for v in chunk])
        _checked.cusrl_accumulate_scalars(table, len(chunk), accumulator.data_ptr() + 4 * start, _stream())
