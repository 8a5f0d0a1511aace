"""Rollout buffer: push, row scatter / splice, flag compaction, minibatch gather and the per-slot record (``csrc/buffer.hip``)."""

from __future__ import annotations

import ctypes
from collections.abc import Sequence

import torch

from cusrl_amd import _native
from cusrl_amd._native import Field, PackedField
from cusrl_amd.ops._common import _checked, _flag, _modified_in_place, _observed, _ptr, _row_bytes, _stream, require_device


def buffer_push(pairs: Sequence[tuple[torch.Tensor, torch.Tensor]], cursor: int, parallelism: int) -> None:
    """``storage[cursor] = step`` for every ``(step [N,...], storage [T,N,...])`` pair in one launch.

    Replaces the per-leaf index_put chain of cusrl/template/buffer.py:134-146.
    """
    for start in range(0, len(pairs), _native.MAX_FIELDS):
        chunk = pairs[start : start + _native.MAX_FIELDS]
        table = (Field * len(chunk))()
        for i, (step, storage) in enumerate(chunk):
            table[i].src = step.data_ptr()
            table[i].dst = storage.data_ptr()
            table[i].row_bytes = _row_bytes(step, 1)
        _observed("cusrl_buffer_push", table, len(chunk), cursor, parallelism,
                nbytes=lambda: sum(2 * step.numel() * step.element_size() for step, _ in chunk))


def make_push_table(leaves: Sequence[tuple[torch.Tensor, tuple]]):
    """Pre-filled ``cusrl_field_t`` array for a fixed set of ``(storage [T, N, ...], step shape)`` leaves: destination
    pointers and row sizes never change between pushes, only the source pointers do."""
    table = (Field * max(len(leaves), 1))()
    for i, (storage, shape) in enumerate(leaves):
        table[i].dst = storage.data_ptr()
        row = storage.element_size()
        for s in shape[1:]:
            row *= s
        table[i].row_bytes = row
    return table


def push_table(table, count: int, cursor: int, parallelism: int, through: tuple | None = None) -> None:
    """Launch ``cusrl_buffer_push`` on a table whose ``src`` pointers were just filled.  ``through`` =
    ``(record tensor, record_bytes, int32 offsets array)``: the leaves with an offset >= 0 are also written into the
    per-slot record from the same registers (``cusrl_buffer_push_through``)."""
    if through is None:
        _observed("cusrl_buffer_push", table, count, cursor, parallelism,
                nbytes=lambda: sum(2 * parallelism * table[i].row_bytes for i in range(count)))
        return
    record, record_bytes, offsets = through
    _observed("cusrl_buffer_push_through", table, count, cursor, parallelism, record.data_ptr(), record_bytes, offsets,
            nbytes=lambda: sum((2 + (offsets[i] >= 0)) * parallelism * table[i].row_bytes for i in range(count)))


def _row_elems(storage: torch.Tensor) -> int:
    n = 1
    for d in storage.shape[2:]:
        n *= d
    return n


def _index_vector(indices: torch.Tensor) -> torch.Tensor:
    require_device(indices, "indices")
    if indices.dtype != torch.int64:
        raise TypeError(f"'indices' must be int64, got {indices.dtype}")
    return indices.contiguous()


def _destinations(caller: str, given, leaves: Sequence[torch.Tensor], lead: tuple, rows: int) -> list[torch.Tensor]:
    """The gather's outputs, ``lead + row shape`` per leaf: new tensors, or the ones the caller ``given`` (validated)."""
    if given is None:
        return [torch.empty(lead + tuple(s.shape[2:]), dtype=s.dtype, device=s.device) for s in leaves]
    given = list(given)
    for dst, src in zip(given, leaves):
        if not dst.is_contiguous() or dst.dtype != src.dtype or dst.numel() != rows * _row_elems(src):
            raise ValueError(f"{caller}: an 'out' tensor does not match its leaf (contiguous, same dtype, batch rows)")
    return given


def _field_table(storages: Sequence[torch.Tensor], outputs: Sequence[torch.Tensor]):
    table = (Field * max(len(storages), 1))()
    for slot, src, dst in zip(table, storages, outputs):
        if not src.is_contiguous():
            raise ValueError("buffer leaves must be contiguous [capacity, parallelism, ...] tensors")
        slot.src, slot.dst, slot.row_bytes = src.data_ptr(), dst.data_ptr(), _row_bytes(src, 2)
    return table


def gather_rows(
    storages: Sequence[torch.Tensor],
    indices: torch.Tensor,
    capacity: int,
    parallelism: int,
    temporal: bool = False,
    out: Sequence[torch.Tensor] | None = None,
) -> list[torch.Tensor]:
    """Minibatch gather of every leaf in one launch.

    ``storage.flatten(0, 1)[indices]`` (cusrl/sampler/mini_batch_sampler.py:87-89) or ``storage[:, indices]``
    (``:113-114``) for each ``[T, N, ...]`` leaf.  ``out``: contiguous destinations the caller owns (e.g. two halves of
    one joint batch), one per leaf.
    """
    indices = _index_vector(indices)
    batch = indices.numel()
    rows = batch * (capacity if temporal else 1)
    outputs = _destinations("gather_rows", out, storages, (capacity, batch) if temporal else (batch,), rows)
    if batch == 0:
        return outputs
    for start in range(0, len(storages), _native.MAX_FIELDS):
        chunk = storages[start : start + _native.MAX_FIELDS]
        _observed("cusrl_gather_rows", _field_table(chunk, outputs[start:]), len(chunk), indices.data_ptr(), batch, capacity,
                parallelism, int(temporal), nbytes=lambda: rows * sum(2 * _row_bytes(s, 2) for s in chunk) + batch * 8)
    return outputs


def window_indices(start: torch.Tensor, env: torch.Tensor, length: int, capacity: int, parallelism: int,
                   cursor: int | None) -> torch.Tensor:
    """Flat slots ``[length * B]`` of ``B`` temporal windows (``data[time_indices, env_indices]`` of
    cusrl/sampler/random_sampler.py:101-113 as one index list); ``cursor`` = oldest row of a FULL ring, else None."""
    require_device(start, "start_indices"), require_device(env, "env_indices")
    if start.dtype != torch.int64 or env.dtype != torch.int64 or start.shape != env.shape:
        raise TypeError("window_indices: int64 index vectors of equal length are required")
    start, env = start.contiguous(), env.contiguous()
    out = torch.empty(length * start.numel(), dtype=torch.int64, device=start.device)
    _checked.cusrl_window_indices(start.data_ptr(), env.data_ptr(), out.data_ptr(), start.numel(), length, capacity, parallelism,
            0 if cursor is None else cursor, _stream())
    return out


class RecordPack:
    """Leaves of a rollout buffer interleaved into ONE record per slot, so that a randomly sampled slot costs as few
    128-byte memory lines as possible (MI355X fetches a whole line for a random row of any size <= 128 B, measured:
    profiles/r02/pmc_summary.json).  Two uses:

    * the narrow leaves (1-8 bytes per slot: log-prob, value, reward, next_value, advantage, return, flags): 27 B of the
      ``ppo`` buffer -> one 32-byte record instead of nine separate line fetches;
    * the HOT set — every leaf one training step reads, wide ones included (observation 192 B + action 48 B + log-prob,
      advantage, return 12 B + done 1 B = 253 B -> a 256-byte record = exactly two lines per sampled slot).

    ``build()`` (re)writes the record from the leaves — once per update, after the ``pre_update`` hooks have produced
    their fields; :func:`gather_rows_packed` then reads the record instead of the leaves.  Layout: wide leaves (a
    multiple of 16 bytes) first at 16-byte offsets, then 8/4-byte, 2-byte and 1-byte entries; the record size is the next
    of 16 / 32 / 64 / a multiple of 128 bytes."""

    NARROW = (1, 2, 4, 8)
    MAX_BYTES = 1024

    @staticmethod
    def eligible(storage: torch.Tensor, wide: bool = False) -> bool:
        if not (storage.is_cuda and storage.is_contiguous() and storage.dim() >= 2):
            return False
        width = _row_bytes(storage, 2)
        return width in RecordPack.NARROW or (wide and width % 16 == 0 and 0 < width <= 512 and storage.data_ptr() % 16 == 0)

    @staticmethod
    def _entries(width: int) -> int:
        return 0 if width >= 16 else (2 if width == 8 else 1)

    @staticmethod
    def _size(total: int) -> int:
        return next((size for size in (16, 32, 64) if size >= total), -(-total // 128) * 128)

    @classmethod
    def plan(cls, storages: dict[str, torch.Tensor], hot: Sequence[str] | None = None) -> list[str]:
        """Leaves to pack.  ``hot`` (leaf names) given: exactly those, wide ones included, when they are all eligible and
        fit; otherwise the narrow leaves in storage order while they fit 64 bytes / ``MAX_PACKED`` entries (packing a
        single leaf would only add a copy, so fewer than two means no record at all)."""
        if hot:
            chosen = [name for name in storages if name in hot]
            widths = [_row_bytes(storages[name], 2) for name in chosen]
            if (len(chosen) >= 2 and all(cls.eligible(storages[name], wide=True) for name in chosen)
                    and sum(cls._entries(w) for w in widths) <= _native.MAX_PACKED
                    and sum(1 for w in widths if w >= 16) <= _native.MAX_FIELDS and cls._size(sum(widths)) <= cls.MAX_BYTES):
                return chosen
        chosen, total, entries = [], 0, 0
        for name, storage in storages.items():
            if not cls.eligible(storage):
                continue
            width = _row_bytes(storage, 2)
            slots = cls._entries(width)
            if entries + slots > _native.MAX_PACKED or total + width > 64:
                break
            chosen.append(name)
            total += width
            entries += slots
        return chosen if len(chosen) >= 2 else []

    def __init__(self, storages: dict[str, torch.Tensor]):
        # widest first: wide leaves land on 16-byte offsets, every narrow entry on a multiple of its width
        names = sorted(storages, key=lambda k: -_row_bytes(storages[k], 2))
        self.leaves = {name: storages[name] for name in names}
        first = next(iter(self.leaves.values()))
        self.rows = first.shape[0] * first.shape[1]
        self.offsets: dict[str, int] = {}
        offset = 0
        for name, storage in self.leaves.items():
            if not self.eligible(storage, wide=True) or storage.shape[0] * storage.shape[1] != self.rows:
                raise ValueError(f"leaf '{name}' cannot be packed")
            self.offsets[name] = offset
            offset += _row_bytes(storage, 2)
        self.used_bytes = offset
        self.record_bytes = self._size(offset)
        widths = [_row_bytes(t, 2) for t in self.leaves.values()]
        if self.record_bytes > self.MAX_BYTES or sum(self._entries(w) for w in widths) > _native.MAX_PACKED:
            raise ValueError("the packed leaves exceed one record (1024 bytes / 16 narrow entries)")
        self.record = torch.empty((self.rows, self.record_bytes), dtype=torch.uint8, device=first.device)
        self.key = tuple((name, t.data_ptr(), _row_bytes(t, 2)) for name, t in self.leaves.items())
        self._table = self.packed_table(list(self.leaves))

    def packed_table(self, names: Sequence[str], tensors: Sequence[torch.Tensor] | None = None):
        """``cusrl_packed_field_t`` array of the leaves ``names`` — their place in the record — pointing at the leaves
        themselves (pack) or at ``tensors``, one per name (the gather's destinations)."""
        table = (PackedField * len(names))()
        for slot, name, tensor in zip(table, names, tensors or [self.leaves[name] for name in names]):
            slot.ptr, slot.offset, slot.width = tensor.data_ptr(), self.offsets[name], _row_bytes(self.leaves[name], 2)
        return table

    def build(self, names: Sequence[str] | None = None) -> None:
        """(Re)write the record from the leaves — all of them, or only ``names`` (the leaves that changed since the
        record last held them: the other bytes of every record stay as they are)."""
        if names is None:
            table, count, moved = self._table, len(self.leaves), self.used_bytes
        else:
            chosen = [name for name in self.leaves if name in set(names)]
            if not chosen:
                return
            table, count, moved = self.packed_table(chosen), len(chosen), sum(_row_bytes(self.leaves[name], 2) for name in chosen)
        owned = self._owned_chunks(None if names is None else set(names))
        if owned is not None:
            _observed("cusrl_pack_rows_owned", table, count, self.record.data_ptr(), self.record_bytes, self.rows, owned[0], owned[1],
                    nbytes=lambda: self.rows * 2 * moved)
            return
        _observed("cusrl_pack_rows", table, count, self.record.data_ptr(), self.record_bytes, self.rows,
                nbytes=lambda: self.rows * 2 * moved)

    def _owned_chunks(self, names: set[str] | None) -> tuple[int, int] | None:
        """``(first chunk, chunks)`` when the narrow leaves of this record occupy at most two 16-byte chunks of their own
        (the layout puts them behind the wide leaves, which end on a chunk boundary) and the call writes ALL of them: the
        kernel may then store those chunks whole.  A partial repack must leave the other narrow leaves' bytes alone."""
        narrow = [name for name, storage in self.leaves.items() if _row_bytes(storage, 2) < 16]
        if not narrow or (names is not None and not all(name in names for name in narrow)):
            return None
        start = min(self.offsets[name] for name in narrow)
        if start % 16:
            return None
        chunks = -(-(self.used_bytes - start) // 16)
        return (start // 16, chunks) if chunks <= 2 else None

    def through_offsets(self, leaves: Sequence[str]):
        """int32 array for ``cusrl_buffer_push_through``: the record offset of every pushed leaf that can be written
        through (a wide leaf of this record: whole 16-byte chunks), -1 for the others; None when there is none."""
        offsets = (ctypes.c_int32 * max(len(leaves), 1))()
        any_through = False
        for i, name in enumerate(leaves):
            storage = self.leaves.get(name)
            wide = (storage is not None and _row_bytes(storage, 2) % 16 == 0 and storage.data_ptr() % 16 == 0
                    and storage.shape[1] * _row_bytes(storage, 2) < 2**32)
            offsets[i] = self.offsets[name] if wide else -1
            any_through |= wide
        return offsets if any_through else None


def gather_rows_packed(
    storages: Sequence[torch.Tensor],
    pack: RecordPack | None,
    packed_names: Sequence[str],
    indices: torch.Tensor,
    capacity: int,
    parallelism: int,
    temporal: bool = False,
    out: Sequence[torch.Tensor] | None = None,
    packed_out: Sequence[torch.Tensor] | None = None,
) -> tuple[list[torch.Tensor], list[torch.Tensor]]:
    """:func:`gather_rows` for ``storages`` plus, from the SAME launch, the leaves ``packed_names`` of ``pack`` read
    through its per-slot record (one sector per sampled slot for all of them).  Results are identical to gathering
    the leaves themselves as long as the record is current (``pack.build()`` after the last write to a packed leaf).
    ``out`` / ``packed_out``: destinations the caller owns, one per plain / packed leaf."""
    if not packed_names:
        return gather_rows(storages, indices, capacity, parallelism, temporal, out=out), []
    if len(storages) > _native.MAX_FIELDS:
        raise ValueError("gather_rows_packed: too many plain leaves for one launch")
    indices = _index_vector(indices)
    batch = indices.numel()
    lead = (capacity, batch) if temporal else (batch,)
    rows = batch * (capacity if temporal else 1)
    sources = [pack.leaves[name] for name in packed_names]
    outputs = _destinations("gather_rows_packed", out, storages, lead, rows)
    packed_outputs = _destinations("gather_rows_packed", packed_out, sources, lead, rows)
    if batch == 0:
        return outputs, packed_outputs
    _observed("cusrl_gather_rows_packed", _field_table(storages, outputs), len(storages), pack.record.data_ptr(),
            pack.record_bytes, pack.packed_table(packed_names, packed_outputs), len(packed_names), indices.data_ptr(), batch, capacity,
            parallelism, int(temporal),
            nbytes=lambda: rows * (sum(2 * _row_bytes(s, 2) for s in storages) + sum(2 * _row_bytes(s, 2) for s in sources)) + batch * 8)
    return outputs, packed_outputs


def compact_flags(flags: torch.Tensor, block_counts: torch.Tensor | None = None,
                  count_out: torch.Tensor | None = None, *, scratch: dict | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Ascending flat slots whose flag is set + their number (int32[1]); no host synchronisation.  ``count_out``
    may be a pinned host tensor (the kernel stores the count there with system scope; see :class:`HostCounter`).
    ``scratch`` (a dict the caller keeps) lets a per-step caller reuse the counter and index buffers: the returned
    indices are then only valid until the next call with the same scratch."""
    flags = _flag(flags, "flags")
    n = flags.numel()
    lib = _native.lib()
    recount = block_counts is None
    if scratch is not None and scratch.get("n") == n and scratch.get("device") == flags.device:
        indices = scratch["indices"]
        if recount:
            block_counts = scratch["counts"]
    else:
        if recount:
            block_counts = torch.empty(max(int(lib.cusrl_flag_blocks(n)), 1), dtype=torch.int32, device=flags.device)
        indices = torch.empty(n, dtype=torch.int64, device=flags.device)
        if scratch is not None and recount:
            scratch.update(n=n, device=flags.device, indices=indices, counts=block_counts)
    if count_out is not None:
        if count_out.dtype != torch.int32 or count_out.numel() != 1 or not (count_out.is_cuda or count_out.is_pinned()):
            raise TypeError("'count_out' must be a 1-element int32 tensor on the device or in pinned host memory")
        count = count_out
    else:
        count = torch.empty(1, dtype=torch.int32, device=flags.device)
    _checked.cusrl_compact_flags(flags.data_ptr(), n, block_counts.data_ptr(), int(recount), indices.data_ptr(), count.data_ptr(), _stream())
    return indices, count


def assign_rows(dst: torch.Tensor, indices: torch.Tensor, src: torch.Tensor) -> None:
    """``dst[indices] = src`` for a contiguous ``dst [N, ...]`` and ``src [K, ...]`` of the same dtype (the reset
    observations spliced into the rollout's current observation, environment.py:365-379) — the 16-byte-lane row scatter
    instead of torch's general ``index_put_``."""
    require_device(src, "src"), require_device(dst, "dst"), require_device(indices, "indices")
    if src.dtype != dst.dtype or indices.dtype != torch.int64 or not dst.is_contiguous() or src.shape[1:] != dst.shape[1:]:
        raise TypeError("assign_rows: dtype/layout mismatch")
    K = indices.numel()
    if K == 0:
        return
    if src.shape[0] != K:
        raise ValueError("assign_rows: one source row per index is required")
    src, indices = src.contiguous(), indices.contiguous()
    _checked.cusrl_scatter_rows(src.data_ptr(), indices.data_ptr(), dst.data_ptr(), K, _row_bytes(src, 1), None, _stream())
    _modified_in_place(dst)


def splice_rows(src: torch.Tensor, init: torch.Tensor, indices: torch.Tensor, count: torch.Tensor, done: torch.Tensor,
                dst: torch.Tensor) -> torch.Tensor:
    """``dst = src`` with the reset rows spliced in (``update_observation_and_state``, environment.py:365-379, fused with
    the copy into the next act step's input): ``dst[n] = src[n]`` where ``done[n]`` is clear, ``dst[indices[k]] = init[k]``
    for ``k < count`` (read on the device).  ``done`` and ``(indices, count)`` must come from the same step epilogue."""
    for tensor, name in ((src, "src"), (init, "init"), (indices, "indices"), (count, "count"), (done, "done"), (dst, "dst")):
        require_device(tensor, name)
    N = src.shape[0]
    if (src.dtype != dst.dtype or init.dtype != dst.dtype or src.shape != dst.shape or init.shape != dst.shape
            or not (src.is_contiguous() and init.is_contiguous() and dst.is_contiguous())):
        raise TypeError("splice_rows: src, init and dst must be contiguous tensors of one shape and dtype")
    if indices.dtype != torch.int64 or indices.numel() < N or count.dtype != torch.int32 or count.numel() != 1 or done.numel() != N:
        raise TypeError("splice_rows: indices int64[>= N], count int32[1], done [N] flags are required")
    if dst.data_ptr() in (src.data_ptr(), init.data_ptr()):
        raise ValueError("splice_rows: dst must not alias src or init")
    done = _flag(done, "done")
    _checked.cusrl_splice_rows(src.data_ptr(), init.data_ptr(), indices.data_ptr(), count.data_ptr(), done.data_ptr(),
            dst.data_ptr(), N, _row_bytes(src, 1), _stream())
    _modified_in_place(dst)
    return dst


class HostCounter:
    """A pinned, device-mapped int32 the host polls for a kernel's result.

    ``int(count.item())`` on a device scalar is a device->host copy plus a stream synchronisation — ~30 us on this
    stack even when the GPU is already idle.  A kernel that stores its scalar result straight into pinned host memory
    (system-scope store) lets the host spin on it and continue a few microseconds after the kernel retires."""

    def __init__(self):
        self.tensor = torch.empty(1, dtype=torch.int32).pin_memory()
        self._view = self.tensor.numpy()

    def arm(self) -> torch.Tensor:
        self._view[0] = -1
        return self.tensor

    def wait(self, timeout: float = 0.01) -> int:
        import time

        view, deadline = self._view, None
        while True:
            value = int(view[0])
            if value >= 0:
                return value
            if deadline is None:
                deadline = time.perf_counter() + timeout
            elif time.perf_counter() > deadline:  # something is slow (first launch, profiler): block the usual way
                torch.cuda.current_stream().synchronize()
                value = int(view[0])
                if value < 0:
                    raise RuntimeError("HostCounter: the kernel retired without publishing its count")
                return value


def scatter_rows(src: torch.Tensor, indices: torch.Tensor, dst: torch.Tensor, count: torch.Tensor | None = None) -> None:
    """``dst.flatten(0, 1)[indices] = src`` (cusrl/hook/on_policy/value.py:78).  With ``count`` (a 1-element int32 on
    the device or in pinned host memory) only the first ``min(len(indices), count)`` rows are written — the number is
    read by the kernel, so a fixed-capacity launch can follow an on-device compaction without a host read."""
    require_device(src, "src"), require_device(dst, "dst"), require_device(indices, "indices")
    if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or not (count.is_cuda or count.is_pinned())):
        raise TypeError("'count' must be a 1-element int32 tensor on the device or in pinned host memory")
    if src.dtype != dst.dtype or indices.dtype != torch.int64 or not dst.is_contiguous():
        raise TypeError("scatter_rows: dtype/layout mismatch")
    src, indices = src.contiguous(), indices.contiguous()
    K = indices.numel()
    if K == 0:
        return
    _checked.cusrl_scatter_rows(src.data_ptr(), indices.data_ptr(), dst.data_ptr(), K, _row_bytes(src, 1), _ptr(count), _stream())
    _modified_in_place(dst)
