"""The PPO objective, the differentiable policy terms and the post-update policy statistics (``csrc/ppo_loss.hip``,
``policy_terms.hip``, ``policy_stats.hip``)."""

from __future__ import annotations

from collections.abc import Sequence

import torch

from cusrl_amd import _native
from cusrl_amd.ops._common import _checked, _f32, _observed, _ptr, _stream
from cusrl_amd.ops.gradient import DeferredColumns


LOSS_DEFER = 1  # CUSRL_LOSS_DEFER


class DeferredLoss:
    """Running sums of the objective's five block partials over the replays of ONE captured minibatch step
    (``CUSRL_LOSS_DEFER``): nothing inside an optimizer step reads the loss VALUES — the backward takes a unit gradient —
    so the captured step skips the one-block finalize launch; every block adds its sums to its own row of ``rows``
    (persistent, zero-filled here, outside the capture) and :meth:`drain` forms the per-replay means once per update on
    the host.  ``weights`` = (w_val, w_sur, w_ent) the capture froze.  The value term evaluated by its own launch on the
    critic's stream (:func:`value_loss_fwd_bwd`) keeps its two sums in ``value_rows``: two launches on two streams must not
    read-modify-write the same words."""

    __slots__ = ("storage", "rows", "value_rows", "value_armed", "value_weight", "policy_has_value", "B", "A", "D", "weights", "blocks",
                 "armed")

    def __init__(self, B: int, A: int, D: int, device, categorical: bool):
        self.B, self.A, self.D = B, A, D
        lib = _native.lib()
        self.blocks = int(lib.cusrl_ppo_loss_blocks(B, 0 if categorical else A))
        # (both sets of rows are windows of ONE tensor: staged for the host and reset as one piece)
        policy, value = max(int(lib.cusrl_ppo_loss_num_partials(B)), 1), max(int(lib.cusrl_value_loss_blocks(B, D)), 1)
        self.storage = torch.zeros(policy * 5 + value * 2, dtype=torch.float64, device=device)
        self.rows = self.storage[: policy * 5].view(policy, 5)
        self.value_rows = self.storage[policy * 5 :].view(value, 2)
        self.weights: tuple[float, float, float] | None = None
        self.value_weight: float | None = None
        self.armed = False  # a launch of the (policy / whole) objective has been recorded against `rows`
        self.value_armed = False  # ... of the separate value term against `value_rows`
        self.policy_has_value = True

    MAX_BLOCKS = 256  # beyond this the per-row read-modify-write and the host-side sum stop being negligible

    def sums(self) -> torch.Tensor | None:
        """The five running sums as a device tensor (no host read) and a reset of the rows; None if nothing ran."""
        if not (self.armed or self.value_armed):
            return None
        total = self.rows[: self.blocks].sum(0)
        self.rows.zero_()
        if self.value_armed:  # sums 0 (squared value error) and 4 (value) came from the separate launch
            value = self.value_rows.sum(0)
            self.value_rows.zero_()
            total = torch.stack((value[0], total[1], total[2], total[3], value[1]))
        return total

    def stage(self):
        """``(storage, decode)`` for a batched host read (``Metrics._stage_pending`` snapshots and zeroes ``storage``):
        ``decode(host values of storage)`` gives what :meth:`metrics` gives, under the flags and weights in force NOW."""
        if not (self.armed or self.value_armed):
            return None
        policy_rows, blocks = self.rows.shape[0], self.blocks
        frozen = (self.armed, self.value_armed, self.policy_has_value, self.weights, self.value_weight)

        def decode(host):
            import numpy as np

            flat = np.asarray(host, dtype=np.float64)
            sums = flat[: policy_rows * 5].reshape(policy_rows, 5)[:blocks].sum(0)
            if frozen[1]:
                value = flat[policy_rows * 5 :].reshape(-1, 2).sum(0)
                sums[0], sums[4] = value[0], value[1]
            return self._metrics(sums.tolist(), *frozen)

        return self.storage, decode

    def drain(self, replays: int) -> dict[str, tuple[float, int]] | None:
        """``{metric: (sum over replays of the per-step mean, samples per step)}`` and a reset of the rows."""
        if replays <= 0 or (total := self.sums()) is None:
            return None
        return self.metrics(total.tolist())

    def metrics(self, sums: Sequence[float]) -> dict[str, tuple[float, int]]:
        return self._metrics(sums, self.armed, self.value_armed, self.policy_has_value, self.weights, self.value_weight)

    def _metrics(self, sums, armed, value_armed, policy_has_value, weights, value_weight) -> dict[str, tuple[float, int]]:
        B, D = self.B, self.D
        out: dict[str, tuple[float, int]] = {}
        if value_armed or (armed and policy_has_value):
            w_val = value_weight if value_armed else weights[0]
            out["value_loss"] = (sums[0] / (B * D) * w_val, 1)
        if armed:
            _, w_sur, w_ent = weights
            out["surrogate_loss"] = (-sums[1] / B * w_sur, 1)
            out["entropy_loss"] = (-sums[2] / B * w_ent, 1)
            out["ratio"] = (sums[3] / B, B)
            out["entropy"] = (sums[2] / B, B)
        if "value_loss" in out:
            out["value"] = (sums[4] / B, B)
        return out


def ppo_loss_fwd_bwd(
    advantage: torch.Tensor,
    old_logp: torch.Tensor,
    action: torch.Tensor,
    mean: torch.Tensor,
    std: torch.Tensor,
    ret: torch.Tensor | None,
    curr_value: torch.Tensor | None,
    old_value: torch.Tensor | None,
    *,
    clip: float,
    value_clip: float | None,
    w_sur: float,
    w_val: float,
    w_ent: float,
    want_grads: bool = True,
    deferred: DeferredLoss | None = None,
) -> dict[str, torch.Tensor]:
    """One pass: losses[0:3] = (value, surrogate, entropy) weighted losses, losses[3:6] = means of |logp ratio|, entropy
    and value (the metrics of common.py:45-49 / value.py:139-141), losses[6] = their sum, per-sample logp/entropy/ratios, and the gradients.

    ``std`` is either the ``[B, A]`` matrix or the ``[A]`` vector it repeats (a state-independent std,
    :func:`ppo_loss_accepts_std_vector`): then it is broadcast inside the kernel and ``d_std`` is the ``[A]`` gradient of
    the vector.  ``ret = curr_value = None``: the launch carries no value term (:func:`value_loss_fwd_bwd` evaluates it on
    the critic's stream); ``losses[0]``, ``losses[5]`` are 0 and there is no ``d_value``.

    ``deferred`` (a :class:`DeferredLoss` of this shape): ONE launch, no finalize — ``losses`` is absent from the result,
    the block sums accumulate in ``deferred.rows``, and with a std vector ``d_std`` comes back as
    :class:`DeferredColumns` (the blocks' column sums, reduced by ``assemble_gradients``)."""
    advantage, old_logp = _f32(advantage, "advantage"), _f32(old_logp, "action_logp")
    action, mean, std = _f32(action, "action"), _f32(mean, "mean"), _f32(std, "std")
    no_value = ret is None and curr_value is None
    if not no_value:
        ret, curr_value = _f32(ret, "return"), _f32(curr_value, "curr_value")
    A = mean.shape[-1]
    B = mean.numel() // A
    D = 0 if no_value else ret.shape[-1]
    std_vector = std.dim() == 1 and B != 1
    if std_vector and not (std.numel() == A and ppo_loss_accepts_std_vector(A)):
        raise ValueError("ppo_loss: a std vector must have one entry per action dim (and the action width a multiple of 4, <= 32)")
    if advantage.numel() != B or old_logp.numel() != B or action.shape != mean.shape or (not std_vector and std.numel() != B * A):
        raise ValueError("ppo_loss: inconsistent batch shapes")
    if no_value:
        value_clip = old_value = None
    elif ret.numel() != B * D or curr_value.shape != ret.shape:
        raise ValueError("ppo_loss: return / value shapes differ")
    if value_clip is not None:
        if old_value is None:
            raise ValueError("ppo_loss: the clipped value loss needs the old value")
        old_value = _f32(old_value, "value")
    if deferred is not None and (deferred.B, deferred.A) != (B, A) or (deferred is not None and not no_value and deferred.D != D):
        raise ValueError("ppo_loss: the deferred-loss rows belong to another minibatch shape")
    dev = mean.device
    lib = _native.lib()
    out = {
        "logp": torch.empty(advantage.shape, dtype=torch.float32, device=dev),
        "entropy": torch.empty(advantage.shape, dtype=torch.float32, device=dev),
        "logp_ratio": torch.empty(advantage.shape, dtype=torch.float32, device=dev),
        "ratio": torch.empty(advantage.shape, dtype=torch.float32, device=dev),
    }
    if deferred is None:
        out["losses"] = torch.empty(7, dtype=torch.float32, device=dev)  # 3 weighted losses, 3 metric means, total
    defer_std = deferred is not None and std_vector and want_grads
    if want_grads:
        out["d_mean"] = torch.empty_like(mean)
        if not no_value:
            out["d_value"] = torch.empty_like(curr_value)
        if not defer_std:
            out["d_std"] = torch.empty_like(std)
    if deferred is None:
        partials = torch.empty((int(lib.cusrl_ppo_loss_num_partials(B)), 5), dtype=torch.float64, device=dev)
    else:
        partials = deferred.rows
        deferred.weights, deferred.armed, deferred.policy_has_value = (float(w_val), float(w_sur), float(w_ent)), True, not no_value
    std_partials = (torch.empty((int(lib.cusrl_ppo_loss_std_partial_rows(B)), A), dtype=torch.float32, device=dev)
                    if std_vector and want_grads else None)
    if defer_std:
        out["d_std"] = DeferredColumns(std_partials, int(lib.cusrl_ppo_loss_blocks(B, A)), A, 0, A)

    def ptr(name):
        value = out.get(name)
        return value.data_ptr() if isinstance(value, torch.Tensor) else None

    _observed(
        "cusrl_ppo_loss_fwd_bwd",
        advantage.data_ptr(), old_logp.data_ptr(), action.data_ptr(), mean.data_ptr(), std.data_ptr(),
        _ptr(ret), _ptr(curr_value), _ptr(None if value_clip is None else old_value),
        B, A, D, float(clip), -1.0 if value_clip is None else float(value_clip), float(w_sur), float(w_val), float(w_ent),
        ptr("losses"), ptr("logp"), ptr("entropy"), ptr("logp_ratio"), ptr("ratio"), ptr("d_mean"), ptr("d_std"), ptr("d_value"),
        partials.data_ptr(), 1 if std_vector else B, _ptr(std_partials), LOSS_DEFER if deferred is not None else 0,
        nbytes=lambda: B * (8 + (8 if std_vector else 12) * A + 8 * D + ((4 if std_vector else 8) * A + 4 * D if want_grads else 0) + 16
                           + (4 * D if value_clip is not None else 0)),
    )
    return out


def ppo_loss_categorical_fwd_bwd(
    advantage: torch.Tensor,
    old_logp: torch.Tensor,
    action: torch.Tensor,
    logits: torch.Tensor,
    ret: torch.Tensor,
    curr_value: torch.Tensor,
    old_value: torch.Tensor | None,
    *,
    clip: float,
    value_clip: float | None,
    w_sur: float,
    w_val: float,
    w_ent: float,
    want_grads: bool = True,
    deferred: DeferredLoss | None = None,
) -> dict[str, torch.Tensor]:
    """:func:`ppo_loss_fwd_bwd` for one-hot categorical policies (``action`` one-hot ``[B, A]``, ``logits [B, A]``):
    same ``losses`` layout and per-sample outputs, gradients ``d_logits`` / ``d_value``; ``deferred`` as there."""
    advantage, old_logp = _f32(advantage, "advantage"), _f32(old_logp, "action_logp")
    action, logits = _f32(action, "action"), _f32(logits, "logits")
    no_value = ret is None and curr_value is None  # (the value term from value_loss_fwd_bwd, see ppo_loss_fwd_bwd)
    if not no_value:
        ret, curr_value = _f32(ret, "return"), _f32(curr_value, "curr_value")
    A = logits.shape[-1]
    B = logits.numel() // A
    D = 0 if no_value else ret.shape[-1]
    if advantage.numel() != B or old_logp.numel() != B or action.shape != logits.shape:
        raise ValueError("ppo_loss_categorical: inconsistent batch shapes")
    if no_value:
        value_clip = old_value = None
    elif ret.numel() != B * D or curr_value.shape != ret.shape:
        raise ValueError("ppo_loss_categorical: return / value shapes differ")
    if value_clip is not None:
        if old_value is None:
            raise ValueError("ppo_loss_categorical: the clipped value loss needs the old value")
        old_value = _f32(old_value, "value")
    if deferred is not None and ((deferred.B, deferred.A) != (B, A) or (not no_value and deferred.D != D)):
        raise ValueError("ppo_loss_categorical: the deferred-loss rows belong to another minibatch shape")
    dev = logits.device
    lib = _native.lib()
    out = {name: torch.empty(advantage.shape, dtype=torch.float32, device=dev) for name in ("logp", "entropy", "logp_ratio", "ratio")}
    if deferred is None:
        out["losses"] = torch.empty(7, dtype=torch.float32, device=dev)
        partials = torch.empty((int(lib.cusrl_ppo_loss_num_partials(B)), 5), dtype=torch.float64, device=dev)
    else:
        partials = deferred.rows
        deferred.weights, deferred.armed, deferred.policy_has_value = (float(w_val), float(w_sur), float(w_ent)), True, not no_value
    if want_grads:
        out["d_logits"] = torch.empty_like(logits)
        if not no_value:
            out["d_value"] = torch.empty_like(curr_value)

    def ptr(name):
        return _ptr(out.get(name))

    _observed(
        "cusrl_ppo_loss_categorical_fwd_bwd",
        advantage.data_ptr(), old_logp.data_ptr(), action.data_ptr(), logits.data_ptr(),
        _ptr(ret), _ptr(curr_value), _ptr(None if value_clip is None else old_value), B, A, D, float(clip),
        -1.0 if value_clip is None else float(value_clip), float(w_sur), float(w_val), float(w_ent), ptr("losses"), ptr("logp"),
        ptr("entropy"), ptr("logp_ratio"), ptr("ratio"), ptr("d_logits"), ptr("d_value"), partials.data_ptr(),
        LOSS_DEFER if deferred is not None else 0,
        nbytes=lambda: B * (8 + 8 * A + 8 * D + ((4 * A + 4 * D) if want_grads else 0) + 16 + (4 * D if value_clip is not None else 0)),
    )
    return out


def value_loss_fwd_bwd(ret: torch.Tensor, curr_value: torch.Tensor, old_value: torch.Tensor | None, *, value_clip: float | None,
                       w_val: float, want_grad: bool = True, deferred: DeferredLoss | None = None) -> dict[str, torch.Tensor]:
    """The value term alone (value.py:85-89,121-137), forward and backward in one launch on the CURRENT stream:
    ``losses`` = (weighted value loss, mean of ``curr_value.sum(-1)``) and ``d_value``.  ``deferred``: no finalize launch,
    the block sums accumulate in ``deferred.value_rows`` (and ``losses`` is absent)."""
    ret, curr_value = _f32(ret, "return"), _f32(curr_value, "curr_value")
    if curr_value.shape != ret.shape or ret.dim() < 1:
        raise ValueError("value_loss: return / value shapes differ")
    D = ret.shape[-1]
    B = ret.numel() // max(D, 1)
    if value_clip is not None:
        if old_value is None:
            raise ValueError("value_loss: the clipped value loss needs the old value")
        old_value = _f32(old_value, "value")
        if old_value.numel() != ret.numel():
            raise ValueError("value_loss: return / old value shapes differ")
    if deferred is not None and (deferred.B, deferred.D) != (B, D):
        raise ValueError("value_loss: the deferred-loss rows belong to another minibatch shape")
    dev, lib = ret.device, _native.lib()
    out: dict[str, torch.Tensor] = {}
    if want_grad:
        out["d_value"] = torch.empty_like(curr_value)
    if deferred is None:
        out["losses"] = torch.empty(2, dtype=torch.float32, device=dev)
        partials = torch.empty((max(int(lib.cusrl_value_loss_blocks(B, D)), 1), 2), dtype=torch.float64, device=dev)
    else:
        partials = deferred.value_rows
        deferred.value_armed, deferred.value_weight = True, float(w_val)
    _observed(
        "cusrl_value_loss_fwd_bwd",
        ret.data_ptr(), curr_value.data_ptr(), _ptr(None if value_clip is None else old_value), B, D,
        -1.0 if value_clip is None else float(value_clip), float(w_val), _ptr(out.get("losses")), _ptr(out.get("d_value")),
        partials.data_ptr(), LOSS_DEFER if deferred is not None else 0,
        nbytes=lambda: B * D * (8 + (4 if want_grad else 0) + (4 if value_clip is not None else 0)),
    )
    return out


def ppo_loss_accepts_std_vector(action_dim: int) -> bool:
    """The row-vector form of ``std`` exists for the 16-byte-chunk layout of the loss kernel."""
    return action_dim % 4 == 0 and action_dim // 4 <= 8


def policy_terms_fwd(mean: torch.Tensor, std: torch.Tensor, action: torch.Tensor, old_logp: torch.Tensor):
    """``(logp, entropy, logp_ratio, prob_ratio)``, each ``[..., 1]``, of a Gaussian policy in ONE launch
    (common.py:29-43, distribution.py:207-213).  ``std`` is ``[..., A]`` like ``mean`` or ONE ``[A]`` vector."""
    mean, std, action, old_logp = _f32(mean, "mean"), _f32(std, "std"), _f32(action, "action"), _f32(old_logp, "old_logp")
    A = mean.shape[-1]
    B = mean.numel() // max(A, 1)
    std_rows = 1 if std.dim() == 1 else B
    if action.numel() != B * A or old_logp.numel() != B or std.numel() != std_rows * A:
        raise ValueError("policy_terms: inconsistent shapes")
    outs = [torch.empty(mean.shape[:-1] + (1,), dtype=torch.float32, device=mean.device) for _ in range(4)]
    _observed("cusrl_policy_terms_fwd", mean.data_ptr(), std.data_ptr(), std_rows, action.data_ptr(), old_logp.data_ptr(), B, A,
            *(o.data_ptr() for o in outs), nbytes=lambda: B * (12 * A + 20))
    return tuple(outs)


def _optional_rows(tensor, rows: int, name: str):
    if tensor is None:
        return None
    tensor = _f32(tensor, name)
    if tensor.numel() != rows:
        raise ValueError(f"policy_terms backward: '{name}' has {tensor.numel()} elements, expected {rows}")
    return tensor


def policy_terms_bwd(mean, std, action, ratio, g_logp, g_entropy, g_logp_ratio, g_ratio):
    """``(d_mean, d_std)`` from the gradients wrt the four outputs of :func:`policy_terms_fwd` (any may be None):
    one launch (+ the one-block column-sum finalize for a std vector)."""
    mean, std, action = _f32(mean, "mean"), _f32(std, "std"), _f32(action, "action")
    A = mean.shape[-1]
    B = mean.numel() // max(A, 1)
    std_rows = 1 if std.dim() == 1 else B
    grads = [_optional_rows(g, B, n) for g, n in ((g_logp, "g_logp"), (g_entropy, "g_entropy"), (g_logp_ratio, "g_logp_ratio"),
                                                   (g_ratio, "g_ratio"))]
    ratio = _optional_rows(ratio, B, "ratio")
    d_mean, d_std = torch.empty_like(mean), torch.empty_like(std)
    lib = _native.lib()
    vector = std_rows == 1 and B != 1
    partials = (torch.empty((max(int(lib.cusrl_policy_terms_std_partial_rows(B)), 1), A), dtype=torch.float32, device=mean.device)
                if vector else None)
    _observed("cusrl_policy_terms_bwd", mean.data_ptr(), std.data_ptr(), std_rows, action.data_ptr(), _ptr(ratio),
            *(_ptr(g) for g in grads), B, A, d_mean.data_ptr(), d_std.data_ptr(), _ptr(partials), nbytes=lambda: B * (20 * A + 20))
    return d_mean, d_std


def categorical_terms_fwd(logits: torch.Tensor, action: torch.Tensor, old_logp: torch.Tensor):
    """The same four terms for a one-hot categorical policy (distribution.py:354-362)."""
    logits, action, old_logp = _f32(logits, "logits"), _f32(action, "action"), _f32(old_logp, "old_logp")
    A = logits.shape[-1]
    B = logits.numel() // max(A, 1)
    if action.numel() != B * A or old_logp.numel() != B:
        raise ValueError("categorical_terms: inconsistent shapes")
    outs = [torch.empty(logits.shape[:-1] + (1,), dtype=torch.float32, device=logits.device) for _ in range(4)]
    _observed("cusrl_categorical_terms_fwd", logits.data_ptr(), action.data_ptr(), old_logp.data_ptr(), B, A,
            *(o.data_ptr() for o in outs), nbytes=lambda: B * (8 * A + 20))
    return tuple(outs)


def categorical_terms_bwd(logits, action, ratio, g_logp, g_entropy, g_logp_ratio, g_ratio):
    logits, action = _f32(logits, "logits"), _f32(action, "action")
    A = logits.shape[-1]
    B = logits.numel() // max(A, 1)
    grads = [_optional_rows(g, B, n) for g, n in ((g_logp, "g_logp"), (g_entropy, "g_entropy"), (g_logp_ratio, "g_logp_ratio"),
                                                   (g_ratio, "g_ratio"))]
    ratio = _optional_rows(ratio, B, "ratio")
    d_logits = torch.empty_like(logits)
    _observed("cusrl_categorical_terms_bwd", logits.data_ptr(), action.data_ptr(), _ptr(ratio), *(_ptr(g) for g in grads), B, A,
            d_logits.data_ptr(), nbytes=lambda: B * (12 * A + 20))
    return d_logits


def policy_stats(old_mean: torch.Tensor, old_std: torch.Tensor, new_mean: torch.Tensor, new_std: torch.Tensor,
                 action: torch.Tensor, old_logp: torch.Tensor, advantage: torch.Tensor) -> torch.Tensor:
    """``[mean KL(old || new), mean advantage * exp(logp_new(action) - old_logp), mean new_std]`` of a Gaussian policy
    over a batch (cusrl/hook/on_policy/stats.py:28-40) — a 3-element device tensor from one pass."""
    tensors = [_f32(t, n) for t, n in ((old_mean, "old_mean"), (old_std, "old_std"), (new_mean, "new_mean"), (new_std, "new_std"),
                                       (action, "action"), (old_logp, "old_logp"), (advantage, "advantage"))]
    A = new_mean.shape[-1] if new_mean.dim() else 0
    B = new_mean.numel() // max(A, 1)
    D = advantage.numel() // max(B, 1)
    if min(A, B, D) == 0 or any(t.numel() != B * A for t in tensors[:5]) or tensors[5].numel() != B or tensors[6].numel() != B * D:
        raise ValueError("policy_stats: inconsistent shapes")
    lib = _native.lib()
    dev = new_mean.device
    partials = torch.empty((max(int(lib.cusrl_policy_stats_num_partials(B)), 1), 3), dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _checked.cusrl_policy_stats(*(t.data_ptr() for t in tensors), B, A, D, partials.data_ptr(), out.data_ptr(), _stream())
    return out


def categorical_policy_stats(old_logits: torch.Tensor, new_logits: torch.Tensor, action: torch.Tensor, old_logp: torch.Tensor,
                             advantage: torch.Tensor) -> torch.Tensor:
    """``[mean KL(old || new), mean advantage * exp(logp_new(action) - old_logp), 0]`` of a one-hot categorical policy over
    a batch — the discrete-action form of :func:`policy_stats`."""
    tensors = [_f32(t, n) for t, n in ((old_logits, "old_logits"), (new_logits, "new_logits"), (action, "action"),
                                       (old_logp, "old_logp"), (advantage, "advantage"))]
    A = new_logits.shape[-1] if new_logits.dim() else 0
    B = new_logits.numel() // max(A, 1)
    D = advantage.numel() // max(B, 1)
    if min(A, B, D) == 0 or any(t.numel() != B * A for t in tensors[:3]) or tensors[3].numel() != B or tensors[4].numel() != B * D:
        raise ValueError("categorical_policy_stats: inconsistent shapes")
    lib = _native.lib()
    dev = new_logits.device
    partials = torch.empty((max(int(lib.cusrl_policy_stats_num_partials(B)), 1), 3), dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _checked.cusrl_categorical_policy_stats(*(t.data_ptr() for t in tensors), B, A, D, partials.data_ptr(), out.data_ptr(), _stream())
    return out
