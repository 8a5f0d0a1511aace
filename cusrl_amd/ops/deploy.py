"""The two elementwise ends of a deployed policy's step (``csrc/deploy.hip``): everything in front of the first GEMM as one
launch, everything behind the last one as one launch.  Formulas and argument rules: include/cusrl_hip.h.  ``*_cpu``: the
library's host restatements of the two kernels, over CPU tensors — what the GPU tests compare bits against."""

from __future__ import annotations

import ctypes

import torch

from cusrl_amd import _native
from cusrl_amd._native import check
from cusrl_amd.ops._common import _checked, _modified_in_place, _ptr, _stream

__all__ = ["deploy_epilogue_", "deploy_epilogue_cpu_", "deploy_prologue", "deploy_prologue_cpu", "deploy_supported"]


def deploy_supported(x, *vectors) -> bool:
    """Do the deploy kernels take ``x``?  A contiguous fp32 ``[B, K]`` device matrix, every given vector a contiguous fp32
    ``[K]`` beside it."""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2 and x.shape[1] > 0 and x.dtype == torch.float32
            and x.is_contiguous() and all(_vector(v, x.shape[1], x.device) for v in vectors if v is not None))


def _vector(v, width: int, device) -> bool:
    return (isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.device == device and tuple(v.shape) == (width,)
            and v.is_contiguous())


def _matrix(x, name: str, cuda: bool) -> None:
    if not (isinstance(x, torch.Tensor) and x.is_cuda == cuda and x.dim() == 2 and x.shape[1] > 0 and x.dtype == torch.float32
            and x.is_contiguous()):
        where = "device" if cuda else "CPU"
        raise ValueError(f"{name} must be a contiguous fp32 [B, K] {where} tensor; got {_describe(x)}")


def _vectors(x, name: str, **vectors) -> None:
    for key, v in vectors.items():
        if v is not None and not _vector(v, x.shape[1], x.device):
            raise ValueError(f"{name}: '{key}' must be a contiguous fp32 [{x.shape[1]}] vector beside its matrix; got {_describe(v)}")


def _pair(name: str, first, second, what: str) -> None:
    if (first is None) != (second is None):
        raise ValueError(f"{name}: {what} must be given together")


def _triple(replace):
    """The host array ``{nan, posinf, neginf}`` of a sanitiser (None: no sanitiser)."""
    if replace is None:
        return None
    nan, posinf, neginf = replace
    return (ctypes.c_float * 3)(float(nan), float(posinf), float(neginf))


def _done(done, rows: int, memory, name: str, cuda: bool):
    if done is None:
        return None, None, 0
    if not (isinstance(done, torch.Tensor) and done.dtype in (torch.bool, torch.uint8) and done.is_cuda == cuda
            and done.numel() == rows and done.is_contiguous()):
        raise ValueError(f"{name}: 'done' must be a contiguous bool tensor of {rows} flags beside 'y'; got {_describe(done)}")
    if not (isinstance(memory, torch.Tensor) and memory.dtype == torch.float32 and memory.device == done.device and memory.dim() == 2
            and memory.shape[0] == rows and memory.shape[1] > 0 and memory.is_contiguous()):
        raise ValueError(f"{name}: 'done' needs a contiguous fp32 [{rows}, M] 'memory' beside it; got {_describe(memory)}")
    return done.data_ptr(), memory.data_ptr(), memory.shape[1]


def deploy_prologue(obs: torch.Tensor, replace=None, mean: torch.Tensor | None = None, std: torch.Tensor | None = None,
                    clamp: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """``clamp((nan_to_num(obs) - mean) / std, -clamp, clamp)`` as ONE launch, every part optional: ``replace`` = ``(nan, posinf,
    neginf)`` or None, ``mean`` / ``std`` both or neither, ``clamp`` None (or <= 0) for none.  The bits of ``ops.nan_to_num_``
    followed by ``ops.rms_normalize``.  ``out``: ``obs`` itself or another contiguous fp32 tensor of its shape; by default a new
    one.  There is no torch form behind this entry: operands it does not take raise."""
    _matrix(obs, "deploy_prologue: 'obs'", True)
    _pair("deploy_prologue", mean, std, "'mean' and 'std'")
    _vectors(obs, "deploy_prologue", mean=mean, std=std)
    if out is None:
        out = torch.empty_like(obs)
    elif not (isinstance(out, torch.Tensor) and out.shape == obs.shape and out.dtype == torch.float32 and out.device == obs.device
              and out.is_contiguous()):
        raise ValueError(f"deploy_prologue: 'out' must be a contiguous fp32 tensor shaped like 'obs'; got {_describe(out)}")
    _checked.cusrl_deploy_prologue(obs.data_ptr(), _triple(replace), _ptr(mean), _ptr(std), -1.0 if clamp is None else float(clamp),
                                   out.data_ptr(), obs.shape[0], obs.shape[1], _stream())
    if out.data_ptr() == obs.data_ptr():
        _modified_in_place(out)
    return out


def deploy_epilogue_(y: torch.Tensor, bias: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                     shift: torch.Tensor | None = None, lo: torch.Tensor | None = None, hi: torch.Tensor | None = None,
                     done: torch.Tensor | None = None, memory: torch.Tensor | None = None) -> torch.Tensor:
    """``y = clip((y + bias) * scale + shift, lo, hi)`` in place on ``y [B, A]`` and, with ``done`` (``[B]`` bool), zeros over
    the rows of ``memory [B, M]`` whose flag is set — ONE launch.  The bias, the affine (``scale`` and ``shift``) and the clip
    (``lo`` and ``hi``) are each optional, all ``[A]`` vectors.  Returns ``y``."""
    _matrix(y, "deploy_epilogue_: 'y'", True)
    _pair("deploy_epilogue_", scale, shift, "'scale' and 'shift'")
    _pair("deploy_epilogue_", lo, hi, "'lo' and 'hi'")
    _vectors(y, "deploy_epilogue_", bias=bias, scale=scale, shift=shift, lo=lo, hi=hi)
    done_ptr, memory_ptr, width = _done(done, y.shape[0], memory, "deploy_epilogue_", True)
    _checked.cusrl_deploy_epilogue(y.data_ptr(), _ptr(bias), _ptr(scale), _ptr(shift), _ptr(lo), _ptr(hi), y.shape[0], y.shape[1],
                                   done_ptr, memory_ptr, width, _stream())
    _modified_in_place(y)
    if done is not None:
        _modified_in_place(memory)
    return y


def deploy_prologue_cpu(obs: torch.Tensor, replace=None, mean=None, std=None, clamp: float | None = None) -> torch.Tensor:
    """:func:`deploy_prologue` by the library's host restatement, over CPU tensors."""
    _matrix(obs, "deploy_prologue_cpu: 'obs'", False)
    _pair("deploy_prologue_cpu", mean, std, "'mean' and 'std'")
    _vectors(obs, "deploy_prologue_cpu", mean=mean, std=std)
    out = torch.empty_like(obs)
    check(_native.lib().cusrl_deploy_prologue_cpu(obs.data_ptr(), _triple(replace), _ptr(mean), _ptr(std),
                                                  -1.0 if clamp is None else float(clamp), out.data_ptr(), obs.shape[0], obs.shape[1]),
          "cusrl_deploy_prologue_cpu")
    return out


def deploy_epilogue_cpu_(y: torch.Tensor, bias=None, scale=None, shift=None, lo=None, hi=None, done=None, memory=None) -> torch.Tensor:
    """:func:`deploy_epilogue_` by the library's host restatement, in place over CPU tensors."""
    _matrix(y, "deploy_epilogue_cpu_: 'y'", False)
    _pair("deploy_epilogue_cpu_", scale, shift, "'scale' and 'shift'")
    _pair("deploy_epilogue_cpu_", lo, hi, "'lo' and 'hi'")
    _vectors(y, "deploy_epilogue_cpu_", bias=bias, scale=scale, shift=shift, lo=lo, hi=hi)
    done_ptr, memory_ptr, width = _done(done, y.shape[0], memory, "deploy_epilogue_cpu_", False)
    check(_native.lib().cusrl_deploy_epilogue_cpu(y.data_ptr(), _ptr(bias), _ptr(scale), _ptr(shift), _ptr(lo), _ptr(hi), y.shape[0],
                                                  y.shape[1], done_ptr, memory_ptr, width), "cusrl_deploy_epilogue_cpu")
    return y


def _describe(value) -> str:
    if not isinstance(value, torch.Tensor):
        return type(value).__name__
    return f"{value.dtype} {tuple(value.shape)} on {value.device}{'' if value.is_contiguous() else ' (strided)'}"
