"""The observation history of a frame stack (``csrc/frame_stack.hip``): one launch per push, one per reset.  Layout, padding rules
and argument rules: include/cusrl_hip.h.  ``*_cpu``: the library's host restatements of the two kernels, over CPU tensors — the
host form of ``nn.ObservationStacker`` / ``environment.FrameStack`` and what the GPU tests compare bits against."""

from __future__ import annotations

import operator

import torch

from cusrl_amd import _native
from cusrl_amd._native import check
from cusrl_amd.ops._common import _checked, _modified_in_place, _ptr, _stream

__all__ = ["frame_stack_columns", "frame_stack_padding", "frame_stack_push", "frame_stack_push_cpu", "frame_stack_reset",
           "frame_stack_reset_cpu", "frame_stack_supported"]

_PADDING = {"reset": _native._CONSTANTS["FRAME_STACK_PAD_RESET"], "zero": _native._CONSTANTS["FRAME_STACK_PAD_ZERO"]}
_CHECKED_WIDTH = "_cusrl_frame_stack_width"  # on a column table: the source width its entries were checked against


def frame_stack_padding(padding_type) -> int:
    """The ``CUSRL_FRAME_STACK_PAD_*`` code of gymnasium's ``padding_type`` (``"reset"`` or ``"zero"``)."""
    if padding_type not in _PADDING:
        raise ValueError(f"padding_type must be one of {list(_PADDING)}; got {padding_type!r}")
    return _PADDING[padding_type]


def frame_stack_columns(columns, width: int, device) -> torch.Tensor | None:
    """``columns`` (a sequence of distinct ints in ``[0, width)``; None: every column in place) as the int32 table the kernels read,
    on ``device``.  Checked and uploaded here — call it outside any capture."""
    if columns is None:
        return None
    if isinstance(columns, torch.Tensor):
        columns = columns.detach().cpu().reshape(-1).tolist()
    try:
        columns = list(columns)
        entries = [operator.index(c) for c in columns]
        ok = bool(entries) and not any(isinstance(c, bool) for c in columns)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"'columns' must be a non-empty sequence of ints; got {columns!r}")
    if min(entries) < 0 or max(entries) >= width:
        raise ValueError(f"'columns' must index a {width}-wide observation (0 .. {width - 1}); got {entries}")
    if len(set(entries)) != len(entries):
        raise ValueError(f"'columns' must be distinct; got {entries}")
    table = torch.tensor(entries, dtype=torch.int32, device=device)
    setattr(table, _CHECKED_WIDTH, int(width))
    return table


def frame_stack_supported(H, obs, columns=None) -> bool:
    """Do the frame-stack kernels take these operands?  A contiguous fp32 ``[N, S, K]`` device history, a contiguous fp32
    ``[.., K0]`` matrix beside it and, when given, a contiguous int32 ``[K]`` table beside both (``K == K0`` without one)."""
    if not (isinstance(H, torch.Tensor) and H.is_cuda and H.dim() == 3 and H.dtype == torch.float32 and H.is_contiguous()
            and H.shape[1] > 0 and H.shape[2] > 0):
        return False
    if not (isinstance(obs, torch.Tensor) and obs.device == H.device and obs.dim() == 2 and obs.dtype == torch.float32
            and obs.is_contiguous() and obs.shape[1] > 0):
        return False
    if columns is None:
        return obs.shape[1] == H.shape[2]
    return (isinstance(columns, torch.Tensor) and columns.device == H.device and columns.dtype == torch.int32
            and tuple(columns.shape) == (H.shape[2],) and columns.is_contiguous())


def _history(H, name: str, cuda: bool) -> tuple[int, int, int]:
    if not (isinstance(H, torch.Tensor) and H.is_cuda == cuda and H.dim() == 3 and H.dtype == torch.float32 and H.is_contiguous()):
        where = "device" if cuda else "CPU"
        raise ValueError(f"{name}: 'H' must be a contiguous fp32 [N, S, K] {where} tensor; got {_describe(H)}")
    N, S, K = H.shape
    if S < 1 or K < 1:
        raise ValueError(f"{name}: 'H' needs stack_size >= 1 and at least one column; got {_describe(H)}")
    return N, S, K


def _source(x, key: str, rows: int, H, name: str) -> int:
    if not (isinstance(x, torch.Tensor) and x.device == H.device and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()
            and x.shape[0] == rows and x.shape[1] > 0):
        raise ValueError(f"{name}: '{key}' must be a contiguous fp32 [{rows}, K0] tensor beside 'H'; got {_describe(x)}")
    return x.shape[1]


def _columns(columns, K: int, K0: int, H, name: str):
    if columns is None:
        if K != K0:
            raise ValueError(f"{name}: without 'columns' the history keeps every column, but 'H' is {K} wide and the observation {K0}")
        return None
    if not (isinstance(columns, torch.Tensor) and columns.device == H.device and columns.dtype == torch.int32
            and tuple(columns.shape) == (K,) and columns.is_contiguous()):
        raise ValueError(f"{name}: 'columns' must be a contiguous int32 [{K}] tensor beside 'H'; got {_describe(columns)}")
    if getattr(columns, _CHECKED_WIDTH, None) != K0:  # a table frame_stack_columns did not make for this width: read once
        if columns.is_cuda and torch.cuda.is_current_stream_capturing():
            raise ValueError(f"{name}: an unchecked 'columns' table cannot be read during capture; make it with frame_stack_columns")
        frame_stack_columns(columns, K0, "cpu")
        setattr(columns, _CHECKED_WIDTH, K0)
    return columns


def _out(out, rows: int, S: int, K: int, H, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(rows, S * K, dtype=torch.float32, device=H.device)
    if not (isinstance(out, torch.Tensor) and out.device == H.device and out.dtype == torch.float32 and out.is_contiguous()
            and out.numel() == rows * S * K and out.shape[0] == rows):
        raise ValueError(f"{name}: 'out' must be a contiguous fp32 [{rows}, {S * K}] tensor beside 'H'; got {_describe(out)}")
    if out.data_ptr() < H.data_ptr() + H.numel() * 4 and H.data_ptr() < out.data_ptr() + out.numel() * 4:
        raise ValueError(f"{name}: 'out' must be a buffer of its own, it overlaps 'H'")
    return out


def _push(name: str, cuda: bool, H, obs, columns, fresh, padding, out) -> torch.Tensor:
    N, S, K = _history(H, name, cuda)
    K0 = _source(obs, "obs", N, H, name)
    columns = _columns(columns, K, K0, H, name)
    code = frame_stack_padding(padding)
    if fresh is not None and not (isinstance(fresh, torch.Tensor) and fresh.dtype in (torch.bool, torch.uint8) and fresh.device == H.device
                                  and fresh.numel() == N and fresh.is_contiguous()):
        raise ValueError(f"{name}: 'fresh' must be a contiguous bool tensor of {N} flags beside 'H'; got {_describe(fresh)}")
    out = _out(out, N, S, K, H, name)
    arguments = (H.data_ptr(), obs.data_ptr(), _ptr(columns), _ptr(fresh), out.data_ptr(), N, S, K, K0, code)
    if cuda:
        _checked.cusrl_frame_stack_push(*arguments, _stream())
    else:
        check(_native.lib().cusrl_frame_stack_push_cpu(*arguments), "cusrl_frame_stack_push_cpu")
    _modified_in_place(H)
    if fresh is not None:
        _modified_in_place(fresh)
    return out


def _reset(name: str, cuda: bool, H, indices, count, reset_obs, columns, padding, out) -> torch.Tensor:
    N, S, K = _history(H, name, cuda)
    if not (isinstance(indices, torch.Tensor) and indices.device == H.device and indices.dtype == torch.int64 and indices.dim() == 1
            and indices.is_contiguous()):
        raise ValueError(f"{name}: 'indices' must be a contiguous int64 [L] tensor beside 'H'; got {_describe(indices)}")
    L = indices.shape[0]
    if count is not None and not (isinstance(count, torch.Tensor) and count.dtype == torch.int32 and count.numel() == 1
                                  and count.device == H.device):
        raise ValueError(f"{name}: 'count' must be a 1-element int32 tensor beside 'H' or None; got {_describe(count)}")
    K0 = _source(reset_obs, "reset_obs", L, H, name)
    columns = _columns(columns, K, K0, H, name)
    code = frame_stack_padding(padding)
    out = _out(out, L, S, K, H, name)
    arguments = (H.data_ptr(), indices.data_ptr(), _ptr(count), reset_obs.data_ptr(), _ptr(columns), out.data_ptr(), L, N, S, K, K0, code)
    if cuda:
        _checked.cusrl_frame_stack_reset(*arguments, _stream())
    else:
        check(_native.lib().cusrl_frame_stack_reset_cpu(*arguments), "cusrl_frame_stack_reset_cpu")
    _modified_in_place(H)
    return out


def frame_stack_push(H: torch.Tensor, obs: torch.Tensor, columns: torch.Tensor | None = None, fresh: torch.Tensor | None = None,
                     padding: str = "reset", out: torch.Tensor | None = None) -> torch.Tensor:
    """``cusrl_frame_stack_push``, ONE launch: every row of ``H [N, S, K]`` drops its oldest slot and takes ``obs[n, columns]`` as
    its newest, in place; returns the new history as a fresh ``[N, S * K]`` tensor (``out``: another contiguous fp32 buffer of that
    size, never ``H``'s storage).  ``fresh`` (``[N]`` bool): a flagged row is refilled from ``obs`` by ``padding`` (``"reset"``:
    every slot; ``"zero"``: zeros in front of it) instead of shifted, and its flag is cleared.  ``columns``: a
    :func:`frame_stack_columns` table.  There is no torch form behind this entry: operands it does not take raise."""
    return _push("frame_stack_push", True, H, obs, columns, fresh, padding, out)


def frame_stack_reset(H: torch.Tensor, indices: torch.Tensor, count: torch.Tensor | None, reset_obs: torch.Tensor,
                      columns: torch.Tensor | None = None, padding: str = "reset", out: torch.Tensor | None = None) -> torch.Tensor:
    """``cusrl_frame_stack_reset``, ONE launch: for ``j < count`` the history of env ``indices[j]`` is refilled from
    ``reset_obs[j, columns]`` by ``padding``; returns ``[len(indices), S * K]`` rows, row ``j`` the history of env ``indices[j]``
    (for ``j >= count`` as it stands: such rows are dropped by the caller, and ``H`` is not written for them).  ``count``: a
    1-element int32 tensor beside ``H``, read by the launch and never by the host; None: every slot."""
    return _reset("frame_stack_reset", True, H, indices, count, reset_obs, columns, padding, out)


def frame_stack_push_cpu(H, obs, columns=None, fresh=None, padding: str = "reset", out=None) -> torch.Tensor:
    """:func:`frame_stack_push` by the library's host restatement, over CPU tensors."""
    return _push("frame_stack_push_cpu", False, H, obs, columns, fresh, padding, out)


def frame_stack_reset_cpu(H, indices, count, reset_obs, columns=None, padding: str = "reset", out=None) -> torch.Tensor:
    """:func:`frame_stack_reset` by the library's host restatement, over CPU tensors."""
    return _reset("frame_stack_reset_cpu", False, H, indices, count, reset_obs, columns, padding, out)


def _describe(value) -> str:
    if not isinstance(value, torch.Tensor):
        return type(value).__name__
    return f"{value.dtype} {tuple(value.shape)} on {value.device}{'' if value.is_contiguous() else ' (strided)'}"
