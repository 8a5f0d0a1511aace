"""Census and memset surgery of a captured hipGraph (``csrc/api.hip``): host-side walks, no launch, no stream."""

from __future__ import annotations

import ctypes

import torch

from cusrl_amd.ops._common import _checked


def graph_census(graph: "torch.cuda.CUDAGraph") -> dict:
    """What a captured hipGraph is made of (``cusrl_graph_census``): ``{"kernel": n, "memcpy": n, "memset": n, "other": n,
    "names": [mangled kernel names in node order]}``.  ``graph`` must have been created with ``keep_graph=True``."""
    raw = ctypes.c_void_p(int(graph.raw_cuda_graph()))
    counts = (ctypes.c_int64 * 16)()
    need = ctypes.c_int64(0)
    capacity = 1 << 16
    while True:
        names = ctypes.create_string_buffer(capacity)
        _checked.cusrl_graph_census(raw, counts, 16, names, capacity, ctypes.byref(need))
        if need.value <= capacity:
            break
        capacity = need.value
    listed = names.raw[: need.value].decode(errors="replace").split("\n")[:-1]
    return {"kernel": counts[0], "memcpy": counts[1], "memset": counts[2], "other": sum(counts[3:]), "names": listed}


def graph_replace_memsets(graph: "torch.cuda.CUDAGraph") -> int:
    """Turn every memset node of a kept, not yet instantiated hipGraph into a fill-kernel node (``cusrl_graph_replace_memsets``);
    returns how many were replaced."""
    replaced = ctypes.c_int64(0)
    _checked.cusrl_graph_replace_memsets(ctypes.c_void_p(int(graph.raw_cuda_graph())), ctypes.byref(replaced))
    return int(replaced.value)
