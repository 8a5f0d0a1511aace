"""What every kernel family shares: the launch observer, the one launch helper, the stream and the small tensor checks."""

from __future__ import annotations

import torch

from cusrl_amd import _native
from cusrl_amd._native import check


class LaunchObserver:
    """Optional HIP-event bracketing of individual launches, placed directly around the C call (after all host-side
    preparation), on the stream the kernel is launched on.  Used by ``bench.py``; ``None`` in normal operation."""

    def __init__(self, only: set[str] | None = None):
        # timing events are not free on this stack (~20-40 us of stream bubble per pair): observe few launches
        self.only = only
        self.records: dict[str, list[tuple[torch.cuda.Event, torch.cuda.Event, int]]] = {}
        self._open: torch.cuda.Event | None = None

    def begin(self):
        self._open = torch.cuda.Event(enable_timing=True)
        self._open.record()

    def end(self, name: str, nbytes: int):
        event = torch.cuda.Event(enable_timing=True)
        event.record()
        self.records.setdefault(name, []).append((self._open, event, nbytes))


_observer: LaunchObserver | None = None


def set_launch_observer(observer: LaunchObserver | None) -> None:
    global _observer
    _observer = observer


def require_device(tensor: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    if not tensor.is_cuda:
        raise RuntimeError(
            f"cusrl_amd: '{name}' lives on {tensor.device}; the rollout + PPO-update hot path only runs as HIP "
            "kernels on an MI355X device tensor (no CPU fallback exists by design)"
        )
    return tensor


def _f32(tensor: torch.Tensor, name: str) -> torch.Tensor:
    require_device(tensor, name)
    if tensor.dtype != torch.float32:
        raise TypeError(f"'{name}' must be float32, got {tensor.dtype}")
    return tensor if tensor.is_contiguous() else tensor.contiguous()


def _flag(tensor: torch.Tensor, name: str) -> torch.Tensor:
    require_device(tensor, name)
    if tensor.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"'{name}' must have dtype bool, got {tensor.dtype}")
    return tensor if tensor.is_contiguous() else tensor.contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """Handle of torch's current stream on the current device (every launch of this module goes there).  The raw
    lookup skips the ``torch.cuda.Stream`` object the public accessor builds — ~2 us per launch on the host, and the
    rollout loop is host-bound."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _row_bytes(tensor: torch.Tensor, lead_dims: int) -> int:
    n = tensor.element_size()
    for s in tensor.shape[lead_dims:]:
        n *= s
    return n


def _modified_in_place(tensor: torch.Tensor) -> None:
    """Tell torch that a raw kernel wrote into ``tensor``: bumps the version counter every alias shares — what
    ``Buffer`` compares to know whether the per-slot record still mirrors a leaf (and what autograd checks)."""
    torch.autograd.graph.increment_version(tensor)


def _ptr(tensor: torch.Tensor | None) -> int | None:
    """Address of an optional tensor (NULL when absent)."""
    return None if tensor is None else tensor.data_ptr()


def _loss_outputs(device, partials_needed: int | None = None, terms: int | None = None):
    """What a loss pass writes besides its gradients (``csrc/loss_reduce.hpp``): the fp32 loss — a scalar, or one entry per
    term — and the float64 partial sums of its blocks, one row per block the library asks for (at least one) times the terms;
    ``partials_needed`` None: a single-workgroup pass, no partials."""
    loss = torch.empty(() if terms is None else terms, dtype=torch.float32, device=device)
    if partials_needed is None:
        return loss, None
    return loss, torch.empty(max(int(partials_needed), 1) * (terms or 1), dtype=torch.float64, device=device)


class _Checked:
    """``_checked.cusrl_x(..., _stream())``: the status-returning entry point ``cusrl_x`` of the loaded library with ``check`` as
    its ctypes ``errcheck``, so the call itself reports under the symbol's name (``_native.launch_counts["cusrl_x"]`` moves) and
    costs no Python frame of its own.  Each symbol is resolved on first use and kept as an attribute: the library is loaded
    once for the life of the process.  (A function object of its own: ``lib().cusrl_x`` stays unchecked for other callers.)"""

    def __getattr__(self, name: str):
        fn, bound = _native.lib()[name], getattr(_native.lib(), name)
        fn.restype, fn.argtypes, fn.errcheck = bound.restype, bound.argtypes, check
        setattr(self, name, fn)
        return fn


_checked = _Checked()


def _observed(name: str, *args, nbytes) -> None:
    """A launch a :class:`LaunchObserver` can time: ``cusrl_<name>(*args, stream)`` on torch's current stream, reported to
    ``check`` under ``name``.  ``nbytes`` (a callable: the bytes the launch moves, only evaluated when timed) is what the
    observer records; its events sit directly around the C call.  Launches nobody times go through ``_checked``."""
    observer = _observer
    if observer is None or (observer.only is not None and name not in observer.only) or torch.cuda.is_current_stream_capturing():
        getattr(_checked, name)(*args, _stream())
        return
    fn = getattr(_native.lib(), name)  # (unchecked: the closing event is recorded before the status is looked at)
    observer.begin()
    status = fn(*args, _stream())
    observer.end(name, nbytes())
    check(status, name)
