"""GPU parity of every HIP kernel against the CPU oracle and the reference goldens, through the C ABI.

Bar (BASELINE.json north_star): bit-exact for index / byte / copy work and for the GAE recurrence;
1e-5 relative fp32 for reductions and losses (tolerances written at each assert).
"""

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from cusrl_amd import ops as _ops

    return _ops


@pytest.fixture
def option():
    """``option(key, value)``: ``cusrl_set_option`` for the duration of the test (every key it touched goes back to 0 — the kernel's
    own rule — afterwards)."""
    from cusrl_amd import _native

    touched = []

    def set_(key, value):
        touched.append(key)
        _native.set_option(key, value)
        assert _native.get_option(key) == value

    yield set_
    for key in touched:
        _native.set_option(key, 0)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def cases(npz):
    return range(int(npz["num_cases"]))


# ------------------------------------------------------------------------------------------------ a1 push
@pytest.mark.parametrize("N", [1, 7, 64, 4096])
def test_push_all_leaves_bit_exact(ops, N):
    rng = np.random.default_rng(N)
    T = 5
    leaves = {
        "observation": rng.standard_normal((N, 48)).astype(np.float32),
        "action": rng.standard_normal((N, 12)).astype(np.float32),
        "reward": rng.standard_normal((N, 1)).astype(np.float32),
        "done": rng.random((N, 1)) < 0.3,
        "odd": rng.integers(0, 255, (N, 3)).astype(np.uint8),
        "index": rng.integers(0, 1 << 40, (N, 1)).astype(np.int64),
        "half": rng.standard_normal((N, 5)).astype(np.float16),
    }
    storages = {k: torch.zeros((T,) + v.shape, dtype=torch.from_numpy(v).dtype, device=DEV) for k, v in leaves.items()}
    expect = {k: np.zeros((T,) + v.shape, v.dtype) for k, v in leaves.items()}
    for cursor in (3, 0, 4):
        step = {k: (v ^ (cursor % 2 == 1)) if v.dtype == bool else (v + cursor).astype(v.dtype) for k, v in leaves.items()}
        ops.buffer_push([(dev(step[k]), storages[k]) for k in leaves], cursor, N)
        for k in leaves:
            oracle.buffer_push(step[k], expect[k], cursor)
    for k in leaves:
        assert np.array_equal(host(storages[k]), expect[k]), k


def test_push_unaligned_views(ops):
    base = torch.arange(0, 4 * 9 + 1, dtype=torch.float32, device=DEV)
    step = base[1:].view(4, 9)  # 4-byte aligned only
    storage = torch.zeros(3, 4, 9, device=DEV)
    ops.buffer_push([(step, storage)], 1, 4)
    assert torch.equal(storage[1], step) and not storage[0].any() and not storage[2].any()


# ------------------------------------------------------------------------------------------------ a7/a8 gather
@pytest.mark.parametrize("T,N,B", [(24, 64, 384), (3, 5, 15), (2, 4099, 1000), (1, 1, 1)])
def test_gather_every_leaf_bit_exact(ops, T, N, B):
    rng = np.random.default_rng(T * N)
    leaves = [
        rng.standard_normal((T, N, 48)).astype(np.float32),
        rng.standard_normal((T, N, 12)).astype(np.float32),
        rng.standard_normal((T, N, 1)).astype(np.float32),
        rng.random((T, N, 1)) < 0.5,
        rng.integers(0, 1 << 40, (T, N, 1)).astype(np.int64),
        rng.integers(0, 255, (T, N, 3)).astype(np.uint8),
        rng.standard_normal((T, N, 2, 3)).astype(np.float32),
    ]
    idx = rng.permutation(T * N)[:B].astype(np.int64)
    outs = ops.gather_rows([dev(x) for x in leaves], dev(idx), T, N, temporal=False)
    for x, out in zip(leaves, outs):
        assert np.array_equal(host(out), oracle.gather_rows(x, idx)), x.shape
    env_idx = rng.permutation(N)[: max(N // 2, 1)].astype(np.int64)
    outs = ops.gather_rows([dev(x) for x in leaves], dev(env_idx), T, N, temporal=True)
    for x, out in zip(leaves, outs):
        assert np.array_equal(host(out), oracle.gather_rows(x, env_idx, temporal=True)), x.shape


def test_gather_full_size_is_a_permutation(ops):
    # config-2 size: 24 x 4096 slots, 4 minibatches of 24576 — size-independent property: each slot exactly once
    T, N = 24, 4096
    flat = torch.arange(T * N, dtype=torch.int64, device=DEV).view(T, N, 1)
    obs = torch.randn(T, N, 48, device=DEV)
    flags = torch.rand(T, N, 1, device=DEV) < 0.1
    perm = torch.randperm(T * N, device=DEV)
    got = []
    for j in range(4):
        idx = perm[j * 24576 : (j + 1) * 24576]
        f, o, b = ops.gather_rows([flat, obs, flags], idx, T, N)
        assert torch.equal(f.squeeze(-1), idx)
        assert torch.equal(o, obs.flatten(0, 1)[idx]) and torch.equal(b, flags.flatten(0, 1)[idx])
        got.append(f)
    assert torch.equal(torch.cat(got).squeeze(-1).sort().values, torch.arange(T * N, device=DEV))


def test_gather_more_than_max_fields(ops):
    T, N = 2, 8
    leaves = [torch.randn(T, N, k % 5 + 1, device=DEV) for k in range(30)]
    idx = torch.randperm(T * N, device=DEV)[:9]
    for x, out in zip(leaves, ops.gather_rows(leaves, idx, T, N)):
        assert torch.equal(out, x.flatten(0, 1)[idx])


# ------------------------------------------------------------------------------------------------ a7/a8 packed record
def _narrow_leaves(rng, T, N, kinds):
    make = {
        "f32": lambda: rng.standard_normal((T, N, 1)).astype(np.float32),
        "bool": lambda: rng.random((T, N, 1)) < 0.4,
        "i64": lambda: rng.integers(0, 1 << 40, (T, N, 1)).astype(np.int64),
        "f16": lambda: rng.standard_normal((T, N, 1)).astype(np.float16),
        "f32x2": lambda: rng.standard_normal((T, N, 2)).astype(np.float32),
        "u8x2": lambda: rng.integers(0, 255, (T, N, 2)).astype(np.uint8),
    }
    return {f"{kind}_{i}": make[kind]() for i, kind in enumerate(kinds)}


@pytest.mark.parametrize("T,N,B,kinds", [
    (24, 64, 384, ["f32"] * 6 + ["bool"] * 3),                 # the ppo buffer's nine narrow leaves: 27 -> 32 B records
    (3, 5, 15, ["f32", "bool"]),                                # 5 -> 16 B
    (2, 4099, 1000, ["i64", "f32x2", "f32", "f16", "u8x2", "bool", "bool"] + ["f32"] * 7),   # 16 fields, 54 -> 64 B
    (1, 1, 1, ["bool", "bool"]),
])
def test_packed_gather_bit_exact(ops, T, N, B, kinds):
    """cusrl_pack_rows + cusrl_gather_rows_packed against the oracle's plain gather of the same leaves."""
    rng = np.random.default_rng(T * N + len(kinds))
    narrow = _narrow_leaves(rng, T, N, kinds)
    wide = [rng.standard_normal((T, N, 48)).astype(np.float32), rng.standard_normal((T, N, 12)).astype(np.float32)]
    storages = {k: dev(v) for k, v in narrow.items()}
    assert ops.RecordPack.plan(storages) == list(storages)
    pack = ops.RecordPack(storages)
    assert pack.record_bytes in (16, 32, 64) and pack.used_bytes <= pack.record_bytes
    pack.build()
    idx = rng.permutation(T * N)[:B].astype(np.int64)
    names = list(narrow)[::-1]  # any subset, in any order
    outs, packed_outs = ops.gather_rows_packed([dev(x) for x in wide], pack, names, dev(idx), T, N)
    for x, out in zip(wide, outs):
        assert np.array_equal(host(out), oracle.gather_rows(x, idx))
    for name, out in zip(names, packed_outs):
        assert out.dtype == storages[name].dtype
        assert np.array_equal(host(out), oracle.gather_rows(narrow[name], idx)), name
    # temporal ([:, idx]) through the same record, and a record-only launch (no plain leaf at all)
    env_idx = rng.permutation(N)[: max(N // 2, 1)].astype(np.int64)
    outs, packed_outs = ops.gather_rows_packed([], pack, names[:3] or names, dev(env_idx), T, N, temporal=True)
    assert outs == []
    for name, out in zip(names[:3] or names, packed_outs):
        assert np.array_equal(host(out), oracle.gather_rows(narrow[name], env_idx, temporal=True)), name
    # the record follows the leaves only when rebuilt
    first = next(iter(storages))
    storages[first].copy_(dev(narrow[first][::-1].copy()))
    pack.build()
    (_, (again,)) = ops.gather_rows_packed([], pack, [first], dev(idx), T, N)
    assert np.array_equal(host(again), oracle.gather_rows(narrow[first][::-1], idx))


@pytest.mark.parametrize("T,N,B", [(24, 256, 1536), (3, 5, 15), (2, 4099, 1000)])
def test_hot_record_with_wide_leaves_bit_exact(ops, T, N, B):
    """The per-slot record holding WIDE leaves too (observation 192 B, action 48 B, three floats, a flag = 253 -> 256 B,
    what a `ppo` training step reads): pack + gather against the oracle's plain gather of the same leaves."""
    rng = np.random.default_rng(T + N)
    leaves = {
        "observation": rng.standard_normal((T, N, 48)).astype(np.float32),
        "action": rng.standard_normal((T, N, 12)).astype(np.float32),
        "action_logp": rng.standard_normal((T, N, 1)).astype(np.float32),
        "advantage": rng.standard_normal((T, N, 1)).astype(np.float32),
        "return": rng.standard_normal((T, N, 1)).astype(np.float32),
        "done": rng.random((T, N, 1)) < 0.3,
    }
    other = rng.standard_normal((T, N, 3)).astype(np.float32)  # a leaf outside the record, same launch
    storages = {k: dev(v) for k, v in leaves.items()}
    assert ops.RecordPack.plan(storages, hot=list(storages)) == list(storages)
    pack = ops.RecordPack(storages)
    assert pack.record_bytes == 256 and pack.used_bytes == 253
    assert pack.offsets["observation"] == 0 and pack.offsets["action"] == 192 and pack.offsets["done"] == 252
    pack.build()
    record = host(pack.record).reshape(T * N, 256)
    assert np.array_equal(record[:, :192].copy().view(np.float32), leaves["observation"].reshape(T * N, 48))
    assert np.array_equal(record[:, 192:240].copy().view(np.float32), leaves["action"].reshape(T * N, 12))
    assert np.array_equal(record[:, 252].astype(bool), leaves["done"].reshape(-1))
    idx = rng.permutation(T * N)[:B].astype(np.int64)
    names = list(leaves)
    (plain,), packed = ops.gather_rows_packed([dev(other)], pack, names, dev(idx), T, N)
    assert np.array_equal(host(plain), oracle.gather_rows(other, idx))
    for name, out in zip(names, packed):
        assert out.dtype == storages[name].dtype and out.is_contiguous()
        assert np.array_equal(host(out), oracle.gather_rows(leaves[name], idx)), name
    env_idx = rng.permutation(N)[: max(N // 2, 1)].astype(np.int64)
    _, packed = ops.gather_rows_packed([], pack, ["action", "done", "observation"], dev(env_idx), T, N, temporal=True)
    for name, out in zip(["action", "done", "observation"], packed):
        assert np.array_equal(host(out), oracle.gather_rows(leaves[name], env_idx, temporal=True)), name
    # a leaf that does not fit the plan (3 floats = 12 bytes: neither narrow nor a multiple of 16) keeps the narrow record
    assert ops.RecordPack.plan({**storages, "odd": dev(other)}, hot=list(storages) + ["odd"]) == ["action_logp", "advantage", "return", "done"]


def test_pack_with_owned_chunks_equals_the_field_by_field_pack(ops):
    """cusrl_pack_rows_owned (the narrow leaves leave as one 16-byte store per owned chunk) against cusrl_pack_rows on the
    same table: identical records wherever a field lives, zero in the owned chunks' padding, wide leaves untouched; a
    partial repack (one stale leaf) must take the field-by-field form and leave its neighbours' bytes alone."""
    from cusrl_amd import _native

    rng = np.random.default_rng(11)
    T, N = 5, 1031
    leaves = {
        "observation": rng.standard_normal((T, N, 48)).astype(np.float32),
        "action": rng.standard_normal((T, N, 12)).astype(np.float32),
        "action_logp": rng.standard_normal((T, N, 1)).astype(np.float32),
        "advantage": rng.standard_normal((T, N, 1)).astype(np.float32),
        "return": rng.standard_normal((T, N, 1)).astype(np.float32),
        "done": rng.random((T, N, 1)) < 0.3,
    }
    storages = {k: dev(v) for k, v in leaves.items()}
    pack = ops.RecordPack(storages)
    assert pack._owned_chunks(None) == (15, 1) and pack._owned_chunks({"advantage", "return"}) is None
    assert pack._owned_chunks({"action_logp", "advantage", "return", "done", "observation"}) == (15, 1)
    pack.record.fill_(0xAB)
    before = dict(_native.launch_counts)
    pack.build()
    assert _native.launch_counts["cusrl_pack_rows_owned"] == before.get("cusrl_pack_rows_owned", 0) + 1
    owned = host(pack.record).copy()
    pack.record.fill_(0xAB)
    lib = _native.lib()
    assert lib.cusrl_pack_rows(pack._table, len(pack.leaves), pack.record.data_ptr(), 256, T * N, None) == 0
    plain = host(pack.record).copy()
    assert np.array_equal(owned[:, :253], plain[:, :253])
    assert not owned[:, 253:].any() and (plain[:, 253:] == 0xAB).all()  # padding: zero when the chunk is owned
    # a stale single leaf: the other narrow bytes of the chunk stay
    storages["advantage"].mul_(2.0)
    before = dict(_native.launch_counts)
    pack.build(["advantage"])
    assert _native.launch_counts["cusrl_pack_rows"] == before.get("cusrl_pack_rows", 0) + 1
    again = host(pack.record)
    assert np.array_equal(again[:, 244:248].copy().view(np.float32).reshape(-1), (leaves["advantage"] * 2.0).reshape(-1))
    assert np.array_equal(again[:, 240:244], plain[:, 240:244]) and np.array_equal(again[:, 248:253], plain[:, 248:253])
    # two owned chunks: the `ppo` buffer's nine narrow leaves (27 -> 32 B)
    narrow = _narrow_leaves(rng, T, N, ["f32"] * 6 + ["bool"] * 3)
    small = ops.RecordPack({k: dev(v) for k, v in narrow.items()})
    assert small._owned_chunks(None) == (0, 2)
    small.record.fill_(0xCD)
    small.build()
    image = host(small.record)
    for name, offset in small.offsets.items():
        width = narrow[name].dtype.itemsize
        assert np.array_equal(image[:, offset:offset + width].copy().view(narrow[name].dtype).reshape(-1), narrow[name].reshape(-1)), name
    assert not image[:, 27:].any()
    # argument errors, straight through ctypes: a narrow field outside the owned chunk, a wide field over it, bad counts
    table = pack._table
    rec = pack.record.data_ptr()
    assert lib.cusrl_pack_rows_owned(table, len(pack.leaves), rec, 256, T * N, 14, 1, None) == -1
    assert lib.cusrl_pack_rows_owned(table, len(pack.leaves), rec, 256, T * N, 15, 0, None) == -1
    assert lib.cusrl_pack_rows_owned(table, len(pack.leaves), rec, 256, T * N, 15, 3, None) == -1
    assert lib.cusrl_pack_rows_owned(table, len(pack.leaves), rec, 256, T * N, 15, 2, None) == -1   # chunk 16 is past the record
    assert lib.cusrl_pack_rows_owned(table, len(pack.leaves), rec, 256, T * N, 14, 2, None) == -1   # `action` ends in chunk 14
    torch.cuda.synchronize()


def test_packed_gather_argument_errors(ops):
    """Negative return codes of the two entry points, straight through ctypes."""
    from cusrl_amd import _native

    lib = _native.lib()
    leaf = torch.zeros(4, 2, 1, device=DEV)
    record = torch.zeros(8, 16, dtype=torch.uint8, device=DEV)
    out = torch.zeros(3, 1, device=DEV)
    idx = torch.zeros(3, dtype=torch.int64, device=DEV)
    table = (_native.PackedField * 2)()
    table[0].ptr, table[0].offset, table[0].width = leaf.data_ptr(), 0, 4
    table[1].ptr, table[1].offset, table[1].width = leaf.data_ptr(), 2, 4                      # misaligned, overlapping
    assert lib.cusrl_pack_rows(table, 2, record.data_ptr(), 16, 8, None) == -1                # CUSRL_E_INVALID
    table[1].offset = 4
    assert lib.cusrl_pack_rows(table, 2, record.data_ptr(), 24, 8, None) == -1                # record size not a multiple of 16
    assert lib.cusrl_pack_rows(table, 2, record.data_ptr(), 2048, 8, None) == -1              # beyond CUSRL_MAX_RECORD_BYTES
    assert lib.cusrl_pack_rows(table, 41, record.data_ptr(), 16, 8, None) == -2               # CUSRL_E_TOO_MANY
    table[1].width = 3
    assert lib.cusrl_pack_rows(table, 2, record.data_ptr(), 16, 8, None) == -1                # unsupported width
    table[1].width, table[0].ptr = 4, out.data_ptr()
    assert lib.cusrl_gather_rows_packed(None, 0, None, 16, table, 1, idx.data_ptr(), 3, 4, 2, 0, None) == -1   # no record
    assert lib.cusrl_gather_rows_packed(None, 25, record.data_ptr(), 16, table, 1, idx.data_ptr(), 3, 4, 2, 0, None) == -1
    torch.cuda.synchronize()


def test_buffer_gathers_through_the_record_and_lazily(ops):
    """Buffer.prepare_sampling packs the narrow leaves; LazyBatch moves only what is read; results equal plain indexing."""
    from cusrl_amd import _native
    from cusrl_amd.sampler import MiniBatchSampler
    from cusrl_amd.template.buffer import Buffer, LazyBatch

    T, N = 6, 32
    buffer = Buffer(T, N, device=DEV)
    assert buffer.record_threshold_bytes == 128 << 20
    buffer.record_threshold_bytes = 0  # this tiny buffer would gather plainly: force the record
    torch.manual_seed(3)
    for _ in range(T):
        buffer.push({"observation": torch.randn(N, 48, device=DEV), "action_dist": {"mean": torch.randn(N, 12, device=DEV),
                     "std": torch.rand(N, 12, device=DEV)}, "reward": torch.randn(N, 1, device=DEV),
                     "value": torch.randn(N, 1, device=DEV), "done": torch.rand(N, 1, device=DEV) < 0.2})
    sampler = MiniBatchSampler(num_epochs=2, num_mini_batches=2)
    counts = _native.launch_counts
    packed_before, plain_before = counts.get("cusrl_gather_rows_packed", 0), counts.get("cusrl_gather_rows", 0)
    seen = []
    for metadata, batch in sampler(buffer):
        assert isinstance(batch, LazyBatch) and set(dict.keys(batch)) | set(batch._pending) == set(buffer.schema)
        first = not seen
        if not first:
            assert set(batch._pending) == {"action_dist", "value"}   # only what the first pass read is prefetched
        reward, obs, done = batch["reward"], batch["observation"], batch["done"]
        seen.append((reward, obs, done))
        if metadata["epoch_index"] == 1 and metadata["mini_batch_index"] == 1:
            value = batch["value"]                                    # a late reader: one extra launch, still correct
            assert "value" in sampler.hot_fields
        assert "next_observation" not in batch and batch.get("nope", 7) == 7
    assert buffer._pack is not None and set(buffer._pack.leaves) == {"reward", "value", "done"}
    assert counts.get("cusrl_gather_rows_packed", 0) - packed_before == 5 and counts.get("cusrl_gather_rows", 0) == plain_before
    assert counts.get("cusrl_pack_rows", 0) >= 1
    with pytest.raises(RuntimeError, match="never read"):
        batch["action_dist"]                                          # the sampler has moved on
    # values: the union of one epoch's minibatches is the whole buffer
    for a, b in ((0, 1), (2, 3)):
        rewards = torch.cat([seen[a][0], seen[b][0]]).flatten().sort().values
        assert torch.equal(rewards, buffer["reward"].flatten().sort().values)
    # eager form = the reference's: everything gathered at once, plain dict
    eager = MiniBatchSampler(num_epochs=1, num_mini_batches=1, lazy=False)
    torch.manual_seed(11)
    (_, full), = list(eager(buffer))
    torch.manual_seed(11)
    perm = torch.randperm(T * N, device=DEV)
    assert type(full) is dict and torch.equal(full["action_dist"]["std"], buffer["action_dist"]["std"].flatten(0, 1)[perm])
    assert torch.equal(full["done"], buffer["done"].flatten(0, 1)[perm])


def _filled_buffer(T, N, threshold=0):
    from cusrl_amd.template.buffer import Buffer

    buffer = Buffer(T, N, device=DEV)
    buffer.record_threshold_bytes = threshold
    torch.manual_seed(5)
    for _ in range(T):
        buffer.push(_step(N))
    return buffer


def _step(N):
    return {"observation": torch.randn(N, 48, device=DEV), "action": torch.randn(N, 12, device=DEV),
            "action_logp": torch.randn(N, 1, device=DEV), "reward": torch.randn(N, 1, device=DEV),
            "done": torch.rand(N, 1, device=DEV) < 0.2}


def test_push_writes_the_wide_leaves_through_into_the_record(ops):
    """Once the record's layout is known, ``push`` stores the wide leaves (observation 192 B, action 48 B) into their record
    slots from the registers that already hold them (cusrl_buffer_push_through): after a full rollout the record mirrors them
    without any pack, ``prepare_sampling`` only moves the narrow leaves, and the gather returns exactly the leaves' rows."""
    from cusrl_amd import _native

    T, N = 8, 256
    buffer = _filled_buffer(T, N)
    buffer["advantage"] = torch.randn(T, N, 1, device=DEV)
    for _ in range(T):  # (a new field re-plans the steady-state append once)
        buffer.push(_step(N))
    hot = {"observation", "action", "action_logp", "advantage", "done"}
    buffer.prepare_sampling(hot)
    pack = buffer._pack
    assert pack is not None and set(pack.leaves) == hot and pack.record_bytes == 256
    counts, observer = _native.launch_counts, ops.LaunchObserver(only={"cusrl_pack_rows"})
    through_before, plain_before = counts.get("cusrl_buffer_push_through", 0), counts.get("cusrl_buffer_push", 0)
    for _ in range(T):  # the next rollout overwrites every row
        buffer.push(_step(N))
    assert counts["cusrl_buffer_push_through"] - through_before == T and counts.get("cusrl_buffer_push", 0) == plain_before
    # the wide leaves are still mirrored, the pushed narrow ones are not; `advantage` was not pushed at all
    assert buffer._mirrored(pack, "observation") and buffer._mirrored(pack, "action") and buffer._mirrored(pack, "advantage")
    assert not buffer._mirrored(pack, "action_logp") and not buffer._mirrored(pack, "done")
    record = pack.record.view(T * N, 256)
    assert torch.equal(record[:, :192].contiguous().view(torch.float32).view(T, N, 48), buffer.storage["observation"])
    assert torch.equal(record[:, 192:240].contiguous().view(torch.float32).view(T, N, 12), buffer.storage["action"])
    ops.set_launch_observer(observer)
    try:
        buffer.prepare_sampling(hot)
    finally:
        ops.set_launch_observer(None)
    (_, _, moved), = observer.records["cusrl_pack_rows"]
    assert moved == T * N * 2 * (4 + 1)  # action_logp + done only: 5 of the 253 bytes per slot, read + written
    assert buffer._pack is pack and all(buffer._mirrored(pack, key) for key in hot)
    indices = torch.randperm(T * N, device=DEV)[: T * N // 2]
    packed_before = counts.get("cusrl_gather_rows_packed", 0)
    batch = buffer.gather(indices, fields=sorted(hot))
    assert counts["cusrl_gather_rows_packed"] == packed_before + 1
    for key in hot:
        assert torch.equal(batch[key], buffer.storage[key].flatten(0, 1)[indices]), key


def test_an_alias_edited_after_the_pack_is_never_read_stale(ops):
    """``buffer[key]`` hands out the storage tensor itself (buffer.py:119-122); a hook may keep it and edit it whenever it
    likes.  The record notices through the tensor's version counter: the next gather reads that leaf from its storage,
    the next ``prepare_sampling`` re-packs exactly that leaf."""
    from cusrl_amd import _native

    T, N = 4, 128
    buffer = _filled_buffer(T, N)
    hot = {"observation", "action_logp", "reward", "done"}
    buffer.prepare_sampling(hot)
    pack = buffer._pack
    kept = buffer["reward"]  # an alias taken BEFORE ...
    buffer.prepare_sampling(hot)
    assert all(buffer._mirrored(pack, key) for key in hot)  # ... reading is not a write
    kept.mul_(3.0)  # ... and edited AFTER the record was built
    assert not buffer._mirrored(pack, "reward") and buffer._mirrored(pack, "observation")
    indices = torch.randperm(T * N, device=DEV)
    batch = buffer.gather(indices, fields=sorted(hot))
    assert torch.equal(batch["reward"], buffer.storage["reward"].flatten(0, 1)[indices])  # the edited values
    observer = ops.LaunchObserver(only={"cusrl_pack_rows"})
    ops.set_launch_observer(observer)
    try:
        buffer.prepare_sampling(hot)
    finally:
        ops.set_launch_observer(None)
    (_, _, moved), = observer.records["cusrl_pack_rows"]
    assert moved == T * N * 2 * 4 and buffer._mirrored(pack, "reward")  # the one stale leaf, nothing else
    # this package's own in-place kernels announce themselves the same way
    ops.normalize_(buffer["reward"], torch.zeros(1, device=DEV), torch.ones(1, device=DEV))
    assert not buffer._mirrored(pack, "reward")
    # ... and a buffer small enough for the caches does not build a record at all
    small = _filled_buffer(T, N, threshold=128 << 20)
    small.prepare_sampling(hot)
    before = _native.launch_counts.get("cusrl_gather_rows", 0)
    small.gather(indices, fields=sorted(hot))
    assert small._pack is None and _native.launch_counts["cusrl_gather_rows"] == before + 1


# ------------------------------------------------------------------------------------------------ a3 next_value
def test_next_value_vs_reference_goldens(ops, golden):
    g = golden("next_value")

    def critic(state, D):
        base = 0.25 * state.sum(-1, keepdim=True) + 0.5 * state[..., :1]
        return torch.cat([base * (d + 1) for d in range(D)], dim=-1)

    for i in cases(g):
        p = f"c{i}_"
        value, nobs = dev(g[p + "value"]), dev(g[p + "next_observation"])
        term, trunc = dev(g[p + "terminated"]), dev(g[p + "truncated"])
        term_value, bootstrap = g[p + "params"]
        T, N, D = value.shape
        out = torch.full_like(value, float("nan"))
        counts = ops.next_value(value, term, trunc, critic(nobs[-1], D), float(term_value), not bootstrap, out)
        indices, count = ops.compact_flags(trunc, counts)
        k = int(count.item())
        expect_idx = np.flatnonzero(g[p + "truncated"].reshape(-1))
        assert k == expect_idx.size and np.array_equal(host(indices[:k]), expect_idx)
        if bootstrap and k:
            (rows,) = ops.gather_rows([nobs], indices[:k], T, N)
            ops.scatter_rows(critic(rows, D), indices[:k], out)
        np.testing.assert_allclose(host(out), g[p + "next_value"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n", [0, 1, 15, 4096, 4097, 98304, 1_000_003])
def test_compact_flags_ordered(ops, n):
    rng = np.random.default_rng(n)
    flags = rng.random(n) < 0.07
    indices, count = ops.compact_flags(dev(flags) if n else torch.zeros(0, dtype=torch.bool, device=DEV))
    k = int(count.item())
    assert k == int(flags.sum()) and np.array_equal(host(indices[:k]), np.flatnonzero(flags))


# ------------------------------------------------------------------------------------------------ a4/a5 GAE
def test_gae_bit_exact_vs_reference_goldens(ops, golden):
    g = golden("gae")
    for i in cases(g):
        p = f"c{i}_"
        gamma, lamda, lv = g[p + "params"]
        adv, ret, partials = ops.gae(dev(g[p + "reward"]), dev(g[p + "value"]), dev(g[p + "next_value"]),
                                     dev(g[p + "done"]), gamma, lamda, None if lv < 0 else lv)
        assert np.array_equal(host(adv), g[p + "advantage"]), f"case {i}: advantage not bit-exact"
        assert np.array_equal(host(ret), g[p + "return"]), f"case {i}: return not bit-exact"
        T, N, D = g[p + "reward"].shape
        if T * N < 2:
            continue
        var, mean = ops.adv_stats_finalize(partials, T * N)
        np.testing.assert_allclose(host(mean), g[p + "mean"], rtol=1e-5, atol=1e-6)  # 1e-5 rel fp32
        np.testing.assert_allclose(host(var), g[p + "var"], rtol=1e-5)
        ops.normalize_(adv, mean, var)
        np.testing.assert_allclose(host(adv), g[p + "normalized"], rtol=1e-5, atol=1e-6)
        # standalone statistics kernel agrees with the fused one
        var2, mean2 = ops.adv_stats_finalize(ops.col_stats(dev(g[p + "advantage"])), T * N)
        np.testing.assert_allclose(host(var2), host(var), rtol=1e-6)
        np.testing.assert_allclose(host(mean2), host(mean), rtol=1e-6, atol=1e-7)


# (5, 50, 3) and (40, 100, 3): D > 1 with a block size that is no multiple of D, so a block's first channel is not 0 — on the
# one-wave-block path (T <= 32) and on the 256-thread path
@pytest.mark.parametrize("T,N,D", [(24, 4096, 1), (24, 4098, 1), (24, 1000, 2), (3, 5, 4), (1, 64, 1), (40, 256, 1), (5, 50, 3),
                                   (40, 100, 3)])
@pytest.mark.parametrize("lamda_value", [None, 0.9])
def test_gae_bit_exact_vs_oracle(ops, T, N, D, lamda_value):
    rng = np.random.default_rng(T + N + D)
    reward = rng.standard_normal((T, N, D)).astype(np.float32)
    value = rng.standard_normal((T, N, D)).astype(np.float32)
    nv = rng.standard_normal((T, N, D)).astype(np.float32)
    done = rng.random((T, N, 1)) < 0.05
    adv, ret, partials = ops.gae(dev(reward), dev(value), dev(nv), dev(done), 0.99, 0.95, lamda_value)
    oadv, oret = oracle.gae(reward, done, value, nv, 0.99, 0.95, lamda_value)
    assert np.array_equal(host(adv), oadv) and np.array_equal(host(ret), oret)
    var, mean = ops.adv_stats_finalize(partials, T * N)
    ovar, omean = oracle.var_mean(oadv)
    np.testing.assert_allclose(host(mean), omean, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(var), ovar, rtol=1e-5)
    # given identical statistics the apply step is bit-exact (true division, correctly rounded sqrt)
    ops.normalize_(adv, dev(omean), dev(ovar))
    assert np.array_equal(host(adv), oracle.normalize(oadv, omean, ovar))


@pytest.mark.parametrize("policy,block", [("0", "256"), ("5", "256"), ("7", "128"), ("5", "128"), ("7", "256")])
@pytest.mark.parametrize("lamda_value", [None, 0.9])
def test_gae_every_cache_policy_and_block_size_is_bit_exact(ops, option, policy, block, lamda_value):
    """The at-scale launch shapes of round 4 (cusrl_gae: cache policy per stream x block size, profiles/r04/gae_policy.md)
    forced one by one on a rollout large enough to take the 4-columns-per-lane path: a cache policy must not change a bit."""
    T, N = 6, 262144 + 4 * 37  # >= 4 * 256 * 256 columns, not a multiple of a block
    rng = np.random.default_rng(int(policy) * 7 + int(block))
    reward, value, nv = (rng.standard_normal((T, N, 1)).astype(np.float32) for _ in range(3))
    done = rng.random((T, N, 1)) < 0.05
    option("gae_policy", 1 + int(policy))  # (through the C ABI: cusrl_set_option — the library reads no environment variable)
    option("gae_block", int(block))
    adv, ret, partials = ops.gae(dev(reward), dev(value), dev(nv), dev(done), 0.99, 0.95, lamda_value)
    oadv, oret = oracle.gae(reward, done, value, nv, 0.99, 0.95, lamda_value)
    assert np.array_equal(host(adv), oadv) and np.array_equal(host(ret), oret)
    var, mean = ops.adv_stats_finalize(partials, T * N)
    ovar, omean = oracle.var_mean(oadv)
    np.testing.assert_allclose(host(mean), omean, rtol=1e-5, atol=1e-6)  # 1e-5 rel fp32
    np.testing.assert_allclose(host(var), ovar, rtol=1e-5)


def test_gae_beyond_the_infinity_cache_takes_the_streaming_policy_and_stays_bit_exact(ops):
    """No override: 16.8 M slots x 21 B = 352 MB > 256 MB, so the launch itself picks non-temporal inputs / `return`."""
    T, N = 8, 1 << 21
    rng = np.random.default_rng(5)
    reward, value, nv = (rng.standard_normal((T, N, 1)).astype(np.float32) for _ in range(3))
    done = rng.random((T, N, 1)) < 0.02
    adv, ret, _ = ops.gae(dev(reward), dev(value), dev(nv), dev(done), 0.99, 0.95, None)
    oadv, oret = oracle.gae(reward, done, value, nv, 0.99, 0.95, None)
    assert np.array_equal(host(adv), oadv) and np.array_equal(host(ret), oret)


@pytest.mark.parametrize("policy", ["0", "3"])
def test_push_streaming_policy_moves_the_same_bytes(ops, option, policy):
    """cusrl_buffer_push with the non-temporal form forced (it is chosen by footprint beyond the Infinity Cache) against the
    oracle's slab assignment: every leaf, mixed widths, an unaligned one."""
    option("push_policy", 2 if policy == "3" else 1)
    rng = np.random.default_rng(int(policy))
    N, T = 5000, 3
    steps = {"observation": rng.standard_normal((N, 48)).astype(np.float32), "action": rng.standard_normal((N, 12)).astype(np.float32),
             "logp": rng.standard_normal((N, 1)).astype(np.float32), "done": rng.random((N, 1)) < 0.1,
             "odd": rng.integers(0, 255, (N, 3)).astype(np.uint8)}
    storage = {k: torch.zeros((T,) + v.shape, dtype=torch.from_numpy(v).dtype, device=DEV) for k, v in steps.items()}
    expect = {k: np.zeros((T,) + v.shape, v.dtype) for k, v in steps.items()}
    for cursor in (1, 2):
        ops.buffer_push([(dev(v), storage[k]) for k, v in steps.items()], cursor, N)
        for k, v in steps.items():
            oracle.buffer_push(v, expect[k], cursor)
    for k in steps:
        assert np.array_equal(host(storage[k]), expect[k]), k


@pytest.mark.parametrize("rows,D", [(1000, 7), (33, 256)])
def test_col_stats_vs_float64(ops, rows, D):
    """The per-channel block partials against float64 numpy: (1000, 7) is two blocks whose first element is not on channel 0
    (4096 % 7 != 0), (33, 256) has D at the supported limit (one thread per channel, nothing to add up)."""
    rng = np.random.default_rng(rows + D)
    x = (rng.standard_normal((rows, D)) * 3 + 0.5).astype(np.float32)
    partials = ops.col_stats(dev(x))
    assert partials.shape == (2 if rows == 1000 else 3, D, 2)
    x64 = x.astype(np.float64)
    sums = host(partials).sum(0)
    # fp64 sums of values (and squares) that are exact in fp64: n * 2^-53 of the absolute sum, 1e-12 with room to spare
    np.testing.assert_allclose(sums[:, 0], x64.sum(0), rtol=0, atol=1e-12 * np.abs(x64).sum(0).max())
    np.testing.assert_allclose(sums[:, 1], (x64 * x64).sum(0), rtol=1e-12)
    var, mean = ops.adv_stats_finalize(partials, rows)
    np.testing.assert_allclose(host(mean), x64.mean(0), rtol=1e-5, atol=1e-6)  # 1e-5 rel fp32
    np.testing.assert_allclose(host(var), x64.var(0, ddof=1), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("offset", [0, 1])
def test_normalize_entry_points_agree_bit_for_bit(ops, offset):
    """``normalize_``, ``normalize_from_partials_`` and ``normalize_from_gathered_`` (one rank: the merge is the identity) are one
    normalisation behind three sources of the statistics: the same bits from all three, and ``oracle.normalize``'s given the
    same statistics.  1001 rows of D = 1: 16-byte aligned storage takes the float4 body + tail, storage that starts 4 bytes
    past a 16-byte boundary the scalar path."""
    rows = 1001
    data = torch.randn(rows, 1, generator=torch.Generator().manual_seed(rows)) * 3 + 0.5

    def fresh():
        x = torch.empty(rows + 4, device=DEV)[offset : offset + rows].view(rows, 1)
        assert x.data_ptr() % 16 == 4 * offset and x.is_contiguous()
        return x.copy_(data)

    x = fresh()
    partials = ops.col_stats(x)
    var, mean = ops.adv_stats_finalize(partials, rows)
    plain = ops.normalize_(fresh(), mean, var, 1e-8)
    assert np.array_equal(host(plain), oracle.normalize(host(x), host(mean), host(var)))
    single = fresh()
    single_var, single_mean = ops.normalize_from_partials_(single, partials, rows, 1e-8)
    assert torch.equal(single, plain) and torch.equal(single_mean, mean) and torch.equal(single_var, var)
    ranked = fresh()
    ranked_var, ranked_mean = ops.normalize_from_gathered_(ranked, ops.packed_mean_var(mean, var)[None], 1e-8)
    assert torch.equal(ranked, plain) and torch.equal(ranked_mean, mean) and torch.equal(ranked_var, var)


def test_gae_propagates_nonfinite_like_reference(ops):
    # 0 * inf = nan in the reference's `not_done * c * A[t+1]`; the kernel multiplies too instead of selecting
    reward = np.zeros((3, 4, 1), np.float32)
    reward[2, 1] = np.inf
    done = np.zeros((3, 4, 1), bool)
    done[1, 1] = True
    zeros = np.zeros_like(reward)
    adv, _, _ = ops.gae(dev(reward), dev(zeros), dev(zeros), dev(done), 0.9, 0.9, None)
    oadv, _ = oracle.gae(reward, done, zeros, zeros, 0.9, 0.9)
    assert np.array_equal(host(adv), oadv, equal_nan=True)


def test_merge_mean_var_vs_reference_goldens(ops, golden):
    g = golden("merge_mean_var")
    for i in cases(g):
        p = f"c{i}_"
        gathered = dev(np.concatenate([g[p + "means"], g[p + "vars"]], axis=-1))
        D = g[p + "means"].shape[1]
        mean, var = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
        ops.merge_mean_var(gathered, mean, var)
        np.testing.assert_allclose(host(mean), g[p + "mean"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(host(var), g[p + "var"], rtol=1e-6)


# ------------------------------------------------------------------------------------------------ a9-a13 loss
def test_ppo_loss_vs_reference_goldens(ops, golden, gradient_parity):
    g = golden("losses")
    for i in cases(g):
        p = f"c{i}_"
        clip, vclip, w_sur, w_val, w_ent = g[p + "params"]
        out = ops.ppo_loss_fwd_bwd(
            dev(g[p + "advantage"]), dev(g[p + "old_logp"]), dev(g[p + "action"]), dev(g[p + "mean"]), dev(g[p + "std"]),
            dev(g[p + "ret"]), dev(g[p + "curr_value"]), dev(g[p + "old_value"]), clip=clip,
            value_clip=None if vclip < 0 else vclip, w_sur=w_sur, w_val=w_val, w_ent=w_ent)
        B = g[p + "mean"].shape[0]
        scale = 1.0 / B
        np.testing.assert_allclose(host(out["logp"]), g[p + "logp"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(host(out["entropy"]), g[p + "entropy"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(host(out["ratio"]), g[p + "ratio"], rtol=2e-5)
        np.testing.assert_allclose(host(out["logp_ratio"]), g[p + "logp_ratio"], rtol=1e-5, atol=1e-5)
        losses = host(out["losses"])
        np.testing.assert_allclose(losses[0], g[p + "value_loss"], rtol=1e-5)  # 1e-5 rel fp32
        np.testing.assert_allclose(losses[1], g[p + "surrogate"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(losses[2], g[p + "entropy_loss"], rtol=1e-5, atol=1e-8)
        # gradients recorded from the reference's autograd (fp32): 1e-5 of the tensor's largest entry
        for name in ("d_mean", "d_std", "d_value"):
            gradient_parity(f"loss_golden.{name}[{i}]", host(out[name]), g[p + name], 1e-5)


def test_policy_terms_forward_vs_reference_goldens(ops, golden):
    """cusrl_policy_terms_fwd against what the reference's OnPolicyPreparation left in the batch (common.py:29-43)."""
    g = golden("losses")
    for i in cases(g):
        p = f"c{i}_"
        logp, entropy, lr, ratio = ops.policy_terms_fwd(dev(g[p + "mean"]), dev(g[p + "std"]), dev(g[p + "action"]), dev(g[p + "old_logp"]))
        np.testing.assert_allclose(host(logp), g[p + "logp"], rtol=1e-5, atol=1e-5)  # 1e-5 rel fp32
        np.testing.assert_allclose(host(entropy), g[p + "entropy"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(host(lr), g[p + "logp_ratio"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(host(ratio), g[p + "ratio"], rtol=2e-5)


@pytest.mark.parametrize("B,A", [(1, 4), (7, 3), (257, 12), (70001, 12), (4096, 64)])
@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("wanted", [(1, 1, 1, 1), (0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 1, 0)])
def test_policy_terms_vs_oracle(ops, B, A, vector, wanted, gradient_parity):
    """Forward and vector-Jacobian product of the policy-terms op against the float64 restatement; any subset of the four
    outputs may carry a gradient (the others arrive as NULL)."""
    rng = np.random.default_rng(B * 31 + A)
    mean, action = rng.standard_normal((B, A), np.float32), rng.standard_normal((B, A), np.float32)
    std = (rng.random(A if vector else (B, A), np.float32) + 0.5).astype(np.float32)
    # the behaviour policy's log-prob: near the current one, like in an update (ratios around 1, not denormals)
    old_logp = (oracle.policy_terms_f64(mean, std, action, np.zeros((B, 1)))["logp"] + 0.3 * rng.standard_normal((B, 1))).astype(np.float32)
    grads = [rng.standard_normal(B).astype(np.float32) if w else None for w in wanted]
    ref = oracle.policy_terms_f64(mean, std, action, old_logp, *grads)
    logp, entropy, lr, ratio = ops.policy_terms_fwd(dev(mean), dev(std), dev(action), dev(old_logp))
    np.testing.assert_allclose(host(logp), ref["logp"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(entropy), ref["entropy"], rtol=1e-5, atol=1e-6)
    noise = 1e-6 * float(np.abs(ref["logp"]).max())  # a difference of two |logp| ~ A numbers: absolute noise ~ ulp(|logp|)
    np.testing.assert_allclose(host(lr), ref["logp_ratio"], rtol=1e-5, atol=1e-5 + noise)
    np.testing.assert_allclose(host(ratio), ref["ratio"], rtol=2e-5 + noise)  # exp() turns that absolute noise into relative
    d_mean, d_std = ops.policy_terms_bwd(dev(mean), dev(std), dev(action), ratio, *(None if g is None else dev(g) for g in grads))
    gradient_parity(f"policy_terms.d_mean[{B},{A},{vector},{wanted}]", host(d_mean), ref["d_mean"], 1e-5)
    gradient_parity(f"policy_terms.d_std[{B},{A},{vector},{wanted}]", host(d_std), ref["d_std"], 1e-5)


def test_policy_terms_autograd_function_matches_torch_distributions(ops):
    """The op as autograd sees it (hook/on_policy/fused.py) against torch.distributions.Normal differentiated by autograd."""
    from cusrl_amd.hook.on_policy.fused import _PolicyTermsFunction

    torch.manual_seed(3)
    B, A = 513, 12
    mean = torch.randn(B, A, device=DEV, requires_grad=True)
    std = (torch.rand(A, device=DEV) + 0.5).requires_grad_()
    action, old_logp = torch.randn(B, A, device=DEV), torch.randn(B, 1, device=DEV) - A
    weights = [torch.randn(B, 1, device=DEV) for _ in range(4)]
    outs = _PolicyTermsFunction.apply(mean, std, action, old_logp)
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    got = (mean.grad.double().cpu(), std.grad.double().cpu())
    m64, s64 = mean.detach().double().cpu().requires_grad_(), std.detach().double().cpu().requires_grad_()
    dist = torch.distributions.Normal(m64, s64.expand(B, A))
    logp = dist.log_prob(action.double().cpu()).sum(-1, keepdim=True)
    lr = logp - old_logp.double().cpu()
    ref = (logp, dist.entropy().sum(-1, keepdim=True), lr, lr.exp())
    sum((o * w.double().cpu()).sum() for o, w in zip(ref, weights)).backward()
    for name, a, b in (("d_mean", got[0], m64.grad), ("d_std", got[1], s64.grad)):
        assert oracle.gradient_error(a.numpy(), b.numpy()) <= 1e-5, name


@pytest.mark.parametrize("B,A", [(1, 3), (300, 3), (5000, 17)])
@pytest.mark.parametrize("wanted", [(1, 1, 1, 1), (0, 0, 0, 1), (0, 1, 0, 0)])
def test_categorical_terms_vs_oracle(ops, B, A, wanted, gradient_parity):
    rng = np.random.default_rng(B + A)
    logits = rng.standard_normal((B, A), np.float32) * 2
    if B > 1:
        logits[1, 0] = -np.inf  # a masked action: p = 0, contributes nothing, gets zero gradient
    taken = rng.integers(1, A, B)
    action = np.eye(A, dtype=np.float32)[taken]
    old_logp = (rng.standard_normal(B).astype(np.float32) - 1).reshape(B, 1)
    grads = [rng.standard_normal(B).astype(np.float32) if w else None for w in wanted]
    ref = oracle.categorical_terms_f64(logits, action, old_logp, *grads)
    logp, entropy, lr, ratio = ops.categorical_terms_fwd(dev(logits), dev(action), dev(old_logp))
    np.testing.assert_allclose(host(logp), ref["logp"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(entropy), ref["entropy"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(ratio), ref["ratio"], rtol=2e-5)
    d_logits = ops.categorical_terms_bwd(dev(logits), dev(action), ratio, *(None if g is None else dev(g) for g in grads))
    assert np.isfinite(host(d_logits)).all()
    gradient_parity(f"categorical_terms.d_logits[{B},{A},{wanted}]", host(d_logits), ref["d_logits"], 1e-5)


def test_categorical_terms_forward_vs_reference_goldens(ops, golden):
    g = golden("categorical_losses")
    for i in cases(g):
        p = f"c{i}_"
        logp, entropy, lr, ratio = ops.categorical_terms_fwd(dev(g[p + "logits"]), dev(g[p + "action"]), dev(g[p + "old_logp"]))
        np.testing.assert_allclose(host(logp), g[p + "logp"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(host(entropy), g[p + "entropy"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(host(ratio), g[p + "ratio"], rtol=2e-5)


def test_categorical_ppo_loss_vs_reference_goldens(ops, golden, gradient_parity):
    """cusrl_ppo_loss_categorical_fwd_bwd vs the reference's OneHotCategoricalDist + PPO hooks (losses, autograd grads)."""
    g = golden("categorical_losses")
    for i in cases(g):
        p = f"c{i}_"
        clip, vclip, w_sur, w_val, w_ent = g[p + "params"]
        out = ops.ppo_loss_categorical_fwd_bwd(
            dev(g[p + "advantage"]), dev(g[p + "old_logp"]), dev(g[p + "action"]), dev(g[p + "logits"]), dev(g[p + "ret"]),
            dev(g[p + "curr_value"]), dev(g[p + "old_value"]), clip=clip, value_clip=None if vclip < 0 else vclip,
            w_sur=w_sur, w_val=w_val, w_ent=w_ent)
        B = g[p + "logits"].shape[0]
        np.testing.assert_allclose(host(out["logp"]), g[p + "logp"], rtol=1e-5, atol=1e-6)      # 1e-5 rel fp32
        np.testing.assert_allclose(host(out["entropy"]), g[p + "entropy"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(host(out["ratio"]), g[p + "ratio"], rtol=2e-5)
        losses = host(out["losses"])
        np.testing.assert_allclose(losses[0], g[p + "value_loss"], rtol=1e-5)
        np.testing.assert_allclose(losses[1], g[p + "surrogate"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(losses[2], g[p + "entropy_loss"], rtol=1e-5, atol=1e-8)
        assert losses[6] == np.float32(np.float32(losses[0] + losses[1]) + losses[2])
        gradient_parity(f"categorical_golden.d_logits[{i}]", host(out["d_logits"]), g[p + "d_logits"], 1e-5)
        gradient_parity(f"categorical_golden.d_value[{i}]", host(out["d_value"]), g[p + "d_value"], 1e-5)


def kernel_clip_sides(out, reference, clip=0.2):
    """Rows where the kernel's fp32 ratio and the float64 ratio fall on different sides of a clip bound.  Such a row is
    legitimate only within fp32 noise of the bound (asserted); the reference is then evaluated with the kernel's side for
    exactly those rows (``flip_clip_side``) instead of masking them out of the comparison."""
    lo, hi = np.float32(1.0 - clip), np.float32(1.0 + clip)
    ratio_k = host(out["ratio"]).ravel()
    ratio_r = reference["ratio"].ravel()
    flip = ((ratio_k >= lo) & (ratio_k <= hi)) != ((ratio_r >= np.float64(lo)) & (ratio_r <= np.float64(hi)))
    assert (reference["clip_margin"][flip] <= 2e-5).all(), "a row far from the clip bound changed sides"
    return flip


@pytest.mark.parametrize("B,A,D", [(64, 3, 1), (24576, 3, 1), (70001, 18, 2), (5, 64, 1)])
@pytest.mark.parametrize("vclip", [None, 0.2])
def test_categorical_ppo_loss_vs_oracle(ops, B, A, D, vclip, gradient_parity):
    rng = np.random.default_rng(B * A)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    logits, adv, ret = 2.0 * f(B, A), f(B, 1), f(B, D)
    taken = rng.integers(0, A, B)
    action = np.eye(A, dtype=np.float32)[taken]
    curr_value, old_value = ret + 0.3 * f(B, D), ret + 0.3 * f(B, D)
    behaviour = oracle.categorical_ppo_loss(adv, np.zeros((B, 1), np.float32), action, logits + 0.05 * f(B, A), ret, curr_value)
    old_logp = behaviour["logp"]
    kw = dict(clip=0.2, value_clip=vclip, w_sur=1.0, w_val=0.5, w_ent=0.01)
    out = ops.ppo_loss_categorical_fwd_bwd(*(dev(x) for x in (adv, old_logp, action, logits, ret, curr_value, old_value)), **kw)
    ref = oracle.categorical_ppo_loss(adv, old_logp, action, logits, ret, curr_value, old_value, **kw)
    losses = host(out["losses"])
    np.testing.assert_allclose(losses[:3], ref["losses"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(losses[4], ref["entropy"].mean(dtype=np.float64), rtol=1e-5)
    np.testing.assert_allclose(host(out["logp"]), ref["logp"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(out["entropy"]), ref["entropy"], rtol=1e-5, atol=1e-6)
    # gradients against the float64 restatement, 1e-5 of the tensor's largest entry; rows within fp32 noise of a clip
    # bound are compared on the side the kernel took
    flip = kernel_clip_sides(out, ref)
    if flip.any():
        ref = oracle.categorical_ppo_loss(adv, old_logp, action, logits, ret, curr_value, old_value, flip_clip_side=flip, **kw)
    tag = f"[B{B},A{A},D{D},vclip={vclip}]"
    gradient_parity("categorical_oracle.d_logits" + tag, host(out["d_logits"]), ref["d_logits"], 1e-5)
    gradient_parity("categorical_oracle.d_value" + tag, host(out["d_value"]), ref["d_value"], 1e-5)


def test_categorical_ppo_loss_with_masked_actions_stays_finite(ops, gradient_parity):
    """A masked action carries logit = -inf: p = 0, log p = -inf.  torch.distributions.Categorical.entropy — what the
    reference's OneHotCategoricalDist evaluates (distribution.py:332-366) — clamps log p to finfo.min before the product,
    so entropy, loss and every gradient of the row stay finite and the masked logits receive exactly zero gradient."""
    rng = np.random.default_rng(17)
    B, A = 3000, 6
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    logits, adv, ret = 2.0 * f(B, A), f(B, 1), f(B, 1)
    masked = rng.random((B, A)) < 0.3
    masked[:, 0] = False  # at least one live action per row
    logits[masked] = -np.inf
    live = np.where(masked, -np.inf, rng.random((B, A)))
    action = np.eye(A, dtype=np.float32)[live.argmax(-1)]  # the taken action is never a masked one
    curr_value = ret + 0.3 * f(B, 1)
    old_logp = oracle.categorical_ppo_loss(adv, np.zeros((B, 1), np.float32), action, np.where(masked, -np.inf, logits + 0.05 * f(B, A)),
                                           ret, curr_value)["logp"]
    kw = dict(clip=0.2, value_clip=None, w_sur=1.0, w_val=0.5, w_ent=0.01)
    out = ops.ppo_loss_categorical_fwd_bwd(*(dev(x) for x in (adv, old_logp, action, logits, ret, curr_value)), None, **kw)
    ref = oracle.categorical_ppo_loss(adv, old_logp, action, logits, ret, curr_value, **kw)
    for key in ("losses", "logp", "entropy", "ratio", "d_logits", "d_value"):
        assert np.isfinite(host(out[key])).all(), key
    assert (host(out["d_logits"])[masked] == 0).all()
    np.testing.assert_allclose(host(out["losses"])[:3], ref["losses"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(host(out["entropy"]), ref["entropy"], rtol=1e-5, atol=1e-6)
    flip = kernel_clip_sides(out, ref)
    if flip.any():
        ref = oracle.categorical_ppo_loss(adv, old_logp, action, logits, ret, curr_value, flip_clip_side=flip, **kw)
    gradient_parity("categorical_masked.d_logits", host(out["d_logits"]), ref["d_logits"], 1e-5)
    # the same numbers from torch.distributions on the device (the library the reference delegates to)
    z = dev(logits).requires_grad_(True)
    dist = torch.distributions.OneHotCategorical(logits=z)
    entropy = dist.entropy()
    assert torch.isfinite(entropy).all()
    np.testing.assert_allclose(host(out["entropy"]).ravel(), host(entropy), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(out["logp"]).ravel(), host(dist.log_prob(dev(action))), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("B,A,D", [(24576, 12, 1), (1000, 7, 1), (513, 32, 2), (3, 40, 1), (255, 4, 3),
                                   (300, 8, 2), (4096, 16, 1), (1000, 20, 1), (2049, 24, 1), (777, 28, 1),  # every row-group width
                                   (70001, 12, 1)])  # last: > 256 blocks, staged reduction of the block partials
@pytest.mark.parametrize("vclip", [None, 0.2])
def test_ppo_loss_vs_oracle(ops, B, A, D, vclip, gradient_parity):
    rng = np.random.default_rng(B + A)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    mean, action, adv, ret = f(B, A), f(B, A), f(B, 1), f(B, D)
    std = (rng.random((B, A)) + 0.5).astype(np.float32)
    action = mean + std * action  # actions drawn from the policy, so ratios stay O(1) like in training
    curr_value, old_value = ret + 0.3 * f(B, D), ret + 0.3 * f(B, D)
    old_logp, _ = oracle.normal_logp_entropy(action, mean + 0.02 * f(B, A), std)
    kw = dict(clip=0.2, value_clip=vclip, w_sur=1.0, w_val=0.5, w_ent=0.01)
    out = ops.ppo_loss_fwd_bwd(*(dev(x) for x in (adv, old_logp, action, mean, std, ret, curr_value, old_value)), **kw)
    ref = oracle.ppo_loss(adv, old_logp, action, mean, std, ret, curr_value, old_value, **kw)
    losses = host(out["losses"])
    np.testing.assert_allclose(losses[:3], ref["losses"], rtol=1e-5, atol=1e-7)
    # the three minibatch metrics the hooks record (common.py:45-49, value.py:139-141), reduced by the same launch
    # |logp - old_logp| cancels two numbers of magnitude |logp| (up to ~60 for 40 actions): fp32 absolute precision
    np.testing.assert_allclose(losses[3], np.abs(ref["logp"] - old_logp).mean(dtype=np.float64), rtol=1e-5,
                               atol=2e-7 * float(np.abs(ref["logp"]).max()))
    np.testing.assert_allclose(losses[4], ref["entropy"].mean(dtype=np.float64), rtol=1e-5)
    np.testing.assert_allclose(losses[5], curr_value.sum(-1).mean(dtype=np.float64), rtol=1e-5, atol=1e-6)
    assert losses[6] == np.float32(np.float32(losses[0] + losses[1]) + losses[2])  # the total the agent differentiates
    np.testing.assert_allclose(host(out["logp"]), ref["logp"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(out["ratio"]), ref["ratio"], rtol=1e-4)
    # gradients against the float64 evaluation of the same formulas (oracle.ppo_loss_f64 explains why fp32 forms cannot be
    # held to 1e-5 against each other), 1e-5 of the tensor's largest entry; rows within fp32 noise of a clip bound are
    # compared on the side the kernel took instead of being masked out
    ref64 = oracle.ppo_loss_f64(adv, old_logp, action, mean, std, ret, curr_value, old_value, **kw)
    flip = kernel_clip_sides(out, ref64)
    if flip.any():
        ref64 = oracle.ppo_loss_f64(adv, old_logp, action, mean, std, ret, curr_value, old_value, flip_clip_side=flip, **kw)
    tag = f"[B{B},A{A},D{D},vclip={vclip}]"
    for name in ("d_mean", "d_std", "d_value"):
        gradient_parity(f"loss_oracle.{name}{tag}", host(out[name]), ref64[name], 1e-5)
        # ... and the fp32 C restatement is itself that close to float64 (it is the checker of the forward values)
        assert oracle.gradient_error(ref[name], ref64[name]) <= 1e-5 or flip.any()


def test_hot_path_rejects_cpu_tensors(ops):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gae(torch.zeros(2, 2, 1), torch.zeros(2, 2, 1), torch.zeros(2, 2, 1), torch.zeros(2, 2, 1, dtype=torch.bool), 0.9, 0.9, None)


# ------------------------------------------------------------------------------------------------ rollout side
@pytest.mark.parametrize("B,A", [(4096, 12), (7, 5), (1, 1), (1000, 32)])
def test_normal_sample_logp_vs_oracle(ops, B, A):
    rng = np.random.default_rng(B * A)
    mean = rng.standard_normal((B, A)).astype(np.float32)
    std = (rng.random((B, A)) + 0.3).astype(np.float32)
    eps = rng.standard_normal((B, A)).astype(np.float32)
    action, logp = ops.normal_sample_logp(dev(mean), dev(std), dev(eps))
    expect = mean + eps * std  # Normal.rsample(): loc + eps * scale, separately rounded
    assert np.array_equal(host(action), expect)
    ref_logp, _ = oracle.normal_logp_entropy(expect, mean, std)
    np.testing.assert_allclose(host(logp), ref_logp, rtol=1e-5, atol=1e-5)
    assert logp.shape == (B, 1)
    # the acting path's form: std as the [A] vector every row repeats (the launch also emits the repeated matrix the
    # rollout buffer stores) and the policy head's bias added to a bias-free product (the finished mean is emitted too):
    # the same numbers as the plain form on the materialised operands, bit for bit
    vector = std[0].copy()
    bias = rng.standard_normal(A).astype(np.float32)
    raw = (mean - bias).astype(np.float32)
    action_v, logp_v, repeated, finished = ops.normal_sample_logp(dev(raw), dev(vector), dev(eps), repeat_std=True, mean_bias=dev(bias))
    assert np.array_equal(host(repeated), np.repeat(vector[None], B, 0))
    assert np.array_equal(host(finished), raw + bias)
    plain_action, plain_logp = ops.normal_sample_logp(dev(raw + bias), dev(np.repeat(vector[None], B, 0)), dev(eps))
    assert torch.equal(action_v, plain_action) and torch.equal(logp_v, plain_logp)


@pytest.mark.parametrize("B,A", [(8, 3), (4096, 12), (1000, 32), (777, 33), (300, 200), (1, 1)])
def test_categorical_sample_logp_vs_oracle(ops, B, A):
    """Both layouts of the kernel (one lane per row up to 32 categories, one wave per row above): the taken category is
    the winner of the exponential race wherever the race is not a numerical tie, the action is its one-hot row and the
    log-prob is log-softmax at it."""
    from cusrl_amd import _native

    rng = np.random.default_rng(B + A)
    logits = (rng.standard_normal((B, A)) * 2.0).astype(np.float32)
    noise = rng.exponential(1.0, (B, A)).astype(np.float32)
    before = _native.launch_counts.get("cusrl_categorical_sample_logp", 0)
    action, logp = ops.categorical_sample_logp(dev(logits), dev(noise))
    assert _native.launch_counts["cusrl_categorical_sample_logp"] == before + 1
    taken, expect_action, expect_logp, margin = oracle.categorical_sample(logits, noise)
    got = host(action)
    assert action.shape == (B, A) and logp.shape == (B, 1)
    assert np.array_equal(got.sum(-1), np.ones(B)) and set(np.unique(got)) <= {0.0, 1.0}
    clear = margin > 1.0 + 1e-4
    assert clear.mean() > 0.99
    assert np.array_equal(got.argmax(-1)[clear], taken[clear])
    assert np.array_equal(got[clear], expect_action[clear])
    log_softmax = logits - np.log(np.exp(logits - logits.max(-1, keepdims=True)).sum(-1, keepdims=True)) - logits.max(-1, keepdims=True)
    np.testing.assert_allclose(host(logp)[:, 0], log_softmax[np.arange(B), got.argmax(-1)], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(host(logp)[clear], expect_logp[clear], rtol=1e-5, atol=2e-6)


def test_categorical_sample_ties_and_dead_categories(ops):
    """Equal races go to the lower index (first arg-max); a category of probability zero (logit -inf) is never taken."""
    logits = torch.tensor([[0.0, 0.0, 0.0], [1.0, -float("inf"), 1.0], [-float("inf"), 2.0, -float("inf")]], device=DEV)
    noise = torch.ones(3, 3, device=DEV)
    noise[1, 1] = 1e-30
    action, logp = ops.categorical_sample_logp(logits, noise)
    assert host(action).argmax(-1).tolist() == [0, 0, 1]
    np.testing.assert_allclose(host(logp)[:, 0], [np.log(1 / 3), np.log(0.5), 0.0], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("A", [3, 48])
def test_categorical_acting_draws_what_torch_multinomial_draws(ops, A):
    """The acting path of OneHotCategoricalDist takes Exp(1) race variables from torch's generator the way
    torch.multinomial does for one sample, so from the same generator state it takes the same categories as
    ``OneHotCategorical(logits).sample()`` on this device — and the frequencies follow softmax(logits)."""
    from cusrl_amd.nn.distribution import OneHotCategoricalDist

    dist = OneHotCategoricalDist(4, A).to(DEV)
    logits = torch.randn(20000, A, device=DEV) * 1.5
    torch.manual_seed(77)
    reference = torch.distributions.OneHotCategorical(logits=logits, validate_args=False).sample()
    torch.manual_seed(77)
    with torch.no_grad():
        action, logp = dist.sample_from_dist({"logits": logits})
    same = (action.argmax(-1) == reference.argmax(-1)).float().mean().item()
    assert same > 0.9995, same
    expect_logp = torch.log_softmax(logits, -1).gather(-1, action.argmax(-1, keepdim=True))
    assert torch.allclose(logp, expect_logp, rtol=1e-5, atol=2e-6)
    # frequencies of one fixed distribution
    row = torch.tensor([2.0, 0.5, -1.0] + [-3.0] * (A - 3), device=DEV)
    with torch.no_grad():
        draws, _ = dist.sample_from_dist({"logits": row.expand(200000, A).contiguous()})
    freq = draws.mean(0)
    assert torch.allclose(freq, torch.softmax(row, 0), atol=4e-3)


def test_sampling_consumes_the_same_random_stream_as_rsample(ops):
    from cusrl_amd.nn import NormalDist

    dist = NormalDist(4, 3).to(DEV)
    params = {"mean": torch.randn(64, 3, device=DEV), "std": torch.rand(64, 3, device=DEV) + 0.5}
    torch.manual_seed(123)
    with torch.no_grad():
        action, logp = dist.sample_from_dist(params)
    torch.manual_seed(123)
    reference = torch.distributions.Normal(params["mean"], params["std"], validate_args=False)
    expect = reference.rsample()
    assert torch.equal(action, expect)
    assert torch.allclose(logp, reference.log_prob(expect).sum(-1, keepdim=True), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("N,D,R", [(4096, 1, 100), (50, 2, 100), (300, 1, 16), (70000, 1, 64)])
def test_episode_stats_one_launch_matches_reference_bookkeeping(ops, N, D, R):
    """cusrl_episode_stats against the reference's track_step + track_episode (trainer.py:54-76), INCLUDING the ring
    order: finished envs take slots in ascending env index, `(arange(count) + num_episodes) % R`, also across a wrap."""
    rng = np.random.default_rng(N + D)
    episode_rew = torch.zeros(N, D, device=DEV)
    episode_len = torch.zeros(N, 1, device=DEV)
    ring_rew, ring_len = torch.zeros(R, D, device=DEV), torch.zeros(R, 1, device=DEV)
    count = torch.zeros(2, dtype=torch.int64, device=DEV)
    reward_sum = torch.zeros(D, dtype=torch.float64, device=DEV)
    h_rew, h_len = np.zeros((N, D), np.float32), np.zeros((N, 1), np.float32)
    h_ring_rew, h_ring_len = np.zeros((R, D), np.float32), np.zeros((R, 1), np.float32)
    total, h_sum, parity = 0, np.zeros(D), 0
    for step in range(6):
        reward = rng.standard_normal((N, D)).astype(np.float32)
        done = rng.random((N, 1)) < (0.02 if N < 60000 else 0.0005)
        ops.episode_stats(dev(reward), dev(done), episode_rew, episode_len, ring_rew, ring_len, count, reward_sum, parity)
        parity ^= 1
        h_rew += reward
        h_len += 1
        h_sum += reward.astype(np.float64).sum(0)
        indices = np.flatnonzero(done)
        slots = (np.arange(indices.size) + total) % R          # trainer.py:66
        h_ring_rew[slots], h_ring_len[slots] = h_rew[indices], h_len[indices]   # later writes win, like index_put
        h_rew[indices] = 0
        h_len[indices] = 0
        total += indices.size
        assert int(count[parity].item()) == total
    assert np.array_equal(host(episode_rew), h_rew) and np.array_equal(host(episode_len), h_len)
    np.testing.assert_allclose(host(reward_sum), h_sum, rtol=1e-12)
    per_step_max = int(N * (0.02 if N < 60000 else 0.0005) * 3)
    if per_step_max < R:  # (a single step that laps the whole ring would make "later writes win" a race on the device)
        assert np.array_equal(host(ring_rew), h_ring_rew) and np.array_equal(host(ring_len), h_ring_len)


@pytest.mark.parametrize("N,D", [(4096, 1), (777, 2), (65536, 1)])
def test_step_epilogue_is_done_flag_statistics_and_ordered_indices_in_one_launch(ops, N, D):
    """cusrl_step_epilogue vs the three things it replaces: terminated | truncated (actor_critic.py:277), the episode
    bookkeeping (trainer.py:54-76) and get_done_indices (environment.py:356-362) — indices bit-exact and ascending."""
    rng = np.random.default_rng(N)
    R = 100
    episode_rew, episode_len = torch.zeros(N, D, device=DEV), torch.zeros(N, 1, device=DEV)
    ring_rew, ring_len = torch.zeros(R, D, device=DEV), torch.zeros(R, 1, device=DEV)
    count = torch.zeros(2, dtype=torch.int64, device=DEV)
    reward_sum = torch.zeros(D, dtype=torch.float64, device=DEV)
    indices = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    counter = ops.HostCounter()
    h_rew, h_len, total, parity = np.zeros((N, D), np.float32), np.zeros((N, 1), np.float32), 0, 0
    h_ring_rew, h_ring_len = np.zeros((R, D), np.float32), np.zeros((R, 1), np.float32)
    for step in range(5):
        reward = rng.standard_normal((N, D)).astype(np.float32)
        terminated, truncated = rng.random((N, 1)) < 0.004, rng.random((N, 1)) < 0.002
        done = torch.empty(N, 1, dtype=torch.bool, device=DEV)
        ops.step_epilogue(dev(reward), dev(terminated), dev(truncated), done, episode_rew, episode_len, ring_rew, ring_len, count,
                          reward_sum, indices, counter.arm(), parity)
        parity ^= 1
        k = counter.wait(timeout=1.0)
        expect = terminated | truncated
        assert np.array_equal(host(done), expect)
        want = np.flatnonzero(expect)
        assert k == want.size and np.array_equal(host(indices[:k]), want)
        h_rew += reward
        h_len += 1
        slots = (np.arange(want.size) + total) % R
        if want.size <= R:
            h_ring_rew[slots], h_ring_len[slots] = h_rew[want], h_len[want]
        h_rew[want] = 0
        h_len[want] = 0
        total += want.size
        assert int(count[parity].item()) == total
    assert np.array_equal(host(episode_rew), h_rew) and np.array_equal(host(episode_len), h_len)
    if N * 0.006 * 3 < R:
        assert np.array_equal(host(ring_rew), h_ring_rew) and np.array_equal(host(ring_len), h_ring_len)
    lib = __import__("cusrl_amd")._native.lib()
    assert lib.cusrl_step_epilogue_max_envs() == 262144
    args = [None] * 12
    assert lib.cusrl_step_epilogue(*args, 4, 1, 100, 0, None) == -1                      # CUSRL_E_INVALID: null pointers
    ptrs = [t.data_ptr() for t in (episode_rew, done, done, done, episode_rew, episode_len, ring_rew, ring_len, count, reward_sum,
                                   indices, count)]
    assert lib.cusrl_step_epilogue(*ptrs, 4, 1, 100, 2, None) == -1                      # parity must be 0 / 1
    assert lib.cusrl_step_epilogue(*ptrs, 262145, 1, 100, 0, None) == -3                 # CUSRL_E_UNSUPPORTED: too many envs


# ------------------------------------------------------------------------------------------------ MLP backward epilogue
@pytest.mark.parametrize("rows,H", [(24576, 256), (24576, 128), (24576, 12), (24576, 1), (100, 32), (7, 5), (1, 4), (4097, 64)])
@pytest.mark.parametrize("mask", [True, False])
def test_relu_backward_bias_matches_autograd(ops, rows, H, mask):
    torch.manual_seed(rows + H)
    grad = torch.randn(rows, H, device=DEV)
    output = torch.relu(torch.randn(rows, H, device=DEV)) if mask else None
    grad_in, colsum = ops.relu_backward_bias(grad, output)
    expect = torch.ops.aten.threshold_backward(grad, output, 0) if mask else grad
    assert torch.equal(grad_in, expect)  # the mask is exact
    ref = expect.double().sum(0)
    # fp32 accumulation over `rows` terms of magnitude ~1: 1e-5 relative to the column's absolute mass
    torch.testing.assert_close(colsum.double(), ref, rtol=1e-5, atol=1e-5 * float(expect.abs().sum(0).max()))


@pytest.mark.parametrize("n", [92569, 3, 65537, 4096, 0])
@pytest.mark.parametrize("max_norm", [1.0, 1e6, None])
def test_clip_grad_norm_vs_oracle_and_torch(ops, n, max_norm):
    rng = np.random.default_rng(n)
    grad = (rng.standard_normal(n) * 0.05).astype(np.float32)
    expect, total = oracle.clip_grad_norm(grad, max_norm)
    flat = dev(grad)
    norm = ops.clip_grad_norm_(flat, max_norm)
    np.testing.assert_allclose(norm.item(), total, rtol=1e-6)
    if max_norm is None or total <= max_norm:
        np.testing.assert_array_equal(host(flat), grad)  # coefficient clamps to exactly 1: untouched
    else:
        np.testing.assert_allclose(host(flat), expect, rtol=1e-6)
    # same numbers as torch's own clip on the device
    reference = torch.nn.Parameter(dev(grad).clone())
    reference.grad = dev(grad).clone()
    if max_norm is not None and n > 0:
        ref_norm = torch.nn.utils.clip_grad_norm_([reference], max_norm)
        np.testing.assert_allclose(norm.item(), ref_norm.item(), rtol=1e-6)
        torch.testing.assert_close(flat, reference.grad, rtol=1e-6, atol=0)


@pytest.mark.parametrize("rows,K,O", [(24576, 128, 12), (24576, 128, 1), (1000, 64, 3), (4097, 256, 16), (65, 128, 5), (1, 1024, 8)])
def test_narrow_linear_backward_matches_matmul(ops, rows, K, O):
    torch.manual_seed(rows + K + O)
    grad, x, w = torch.randn(rows, O, device=DEV), torch.randn(rows, K, device=DEV), torch.randn(O, K, device=DEV)
    assert ops.narrow_linear_supported(K, O)
    dx, dw, db, none_colsum = ops.narrow_linear_backward(grad, x, w)
    assert none_colsum is None
    g64, x64, w64 = grad.double(), x.double(), w.double()
    torch.testing.assert_close(dx.double(), g64 @ w64, rtol=1e-5, atol=1e-5 * float((g64.abs() @ w64.abs()).max()))
    # fp32 accumulation over `rows` products: 1e-5 relative to the absolute mass of each sum
    torch.testing.assert_close(dw.double(), g64.t() @ x64, rtol=1e-5, atol=1e-5 * float((g64.abs().t() @ x64.abs()).max()))
    torch.testing.assert_close(db.double(), g64.sum(0), rtol=1e-5, atol=1e-5 * float(g64.abs().sum(0).max()))
    none, dw2, db2, _ = ops.narrow_linear_backward(grad, x, w, need_input_grad=False)
    assert none is None and torch.equal(dw2, dw) and torch.equal(db2, db)  # deterministic summation order
    # input = a ReLU output: the same pass masks dX by (x > 0) and returns its column sums
    relu_x = torch.relu(x)
    mdx, mdw, mdb, colsum = ops.narrow_linear_backward(grad, relu_x, w, relu_input=True)
    plain_dx, plain_dw, plain_db, _ = ops.narrow_linear_backward(grad, relu_x, w)
    expect = plain_dx * (relu_x > 0)
    assert torch.equal(mdx, expect) and torch.equal(mdw, plain_dw) and torch.equal(mdb, plain_db)
    torch.testing.assert_close(colsum.double(), expect.double().sum(0), rtol=1e-5, atol=1e-5 * float(expect.abs().sum(0).max()) + 1e-12)
    assert not ops.narrow_linear_supported(48, 12) and not ops.narrow_linear_supported(128, 17)


def _plain_layers(mlp, x):
    """The Linear / ReLU stack of ``mlp`` through torch's own ops only (``F.linear`` = addmm, ``torch.relu``; autograd's
    AddmmBackward / threshold_backward / ATen ``sum``) — since round 5 ``cusrl_amd.nn.Linear`` takes the hand-written backward
    at every batch size, so ``mlp.layers(x)`` is no longer an independent reference.  (Bounds of the comparisons below: a
    pre-activation within fp32 rounding of zero may fall on either side of the ReLU in the two evaluations, which moves a
    weight-gradient row by ~1 / rows of its largest entry.)"""
    for layer in mlp.layers:
        x = torch.nn.functional.linear(x, layer.weight, layer.bias) if isinstance(layer, torch.nn.Linear) else torch.relu(x)
    return x


def test_head_behind_relu_backbone_matches_plain_autograd():
    """Backbone (Linear-ReLU x2) + narrow heads: the head's backward also plays the last ReLU's backward; with two
    heads on the same features autograd accumulates their gradients and the shortcut must void itself."""
    from cusrl_amd.nn.module import Linear, Mlp

    torch.manual_seed(5)
    mlp = Mlp(48, (256, 128), ends_with_activation=True).to(DEV)
    heads = [Linear(128, 12).to(DEV), Linear(128, 1).to(DEV)]
    x = torch.randn(8192, 48, device=DEV)
    for used in ([0], [1], [0, 1]):
        params = list(mlp.parameters()) + [p for i in used for p in heads[i].parameters()]
        feat = mlp(x)
        loss = sum(heads[i](feat).square().sum() for i in used)
        got = torch.autograd.grad(loss, params)
        feat = _plain_layers(mlp, x)
        loss = sum(torch.nn.functional.linear(feat, heads[i].weight, heads[i].bias).square().sum() for i in used)
        want = torch.autograd.grad(loss, params)
        for a, b in zip(got, want):
            torch.testing.assert_close(a, b, rtol=2e-4, atol=1e-4 * float(b.abs().max()))


@pytest.mark.parametrize("K", [32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("rows", [1, 7, 24576, 98304 + 3])
def test_one_output_linear_forward_vs_float64(ops, rows, K):
    """cusrl_narrow_linear_fwd (value head / discriminator logit: cusrl/nn/module/critic.py:87-88, hook/auxiliary/amp.py:138-147):
    ``x @ w.T + b`` of a one-output layer as a row dot product, against float64 — within fp32 rounding of the sum of |x| |w|."""
    from cusrl_amd import _native

    torch.manual_seed(rows + K)
    x, w, b = torch.randn(rows, K, device=DEV), torch.randn(1, K, device=DEV), torch.randn(1, device=DEV)
    assert ops.narrow_linear_forward_supported(x, w)
    before = _native.launch_counts.get("cusrl_narrow_linear_fwd", 0)
    for bias in (b, None):
        got = ops.narrow_linear_forward(x, w, bias)
        want = x.double() @ w.double().t() + (0.0 if bias is None else bias.double())
        scale = (x.abs().double() @ w.abs().double().t())
        assert got.shape == (rows, 1)
        assert float(((got.double() - want).abs() / scale.clamp_min(1e-30)).max()) < 4e-7
    assert _native.launch_counts["cusrl_narrow_linear_fwd"] == before + 2
    assert not ops.narrow_linear_forward_supported(x, torch.randn(2, K, device=DEV))            # wider heads: the library GEMM
    assert not ops.narrow_linear_forward_supported(torch.randn(rows, 48, device=DEV), torch.randn(1, 48, device=DEV))
    assert not ops.narrow_linear_forward_supported(x.t().contiguous().t(), w) or rows == 1 or K == 1   # a strided view


def test_one_output_head_takes_the_row_dot_launch_in_both_modes():
    """``cusrl_amd.nn.Linear`` with one output: the forward is the row-dot launch with and without autograd, the backward the
    narrow-head pass; values and gradients against torch's own linear."""
    from cusrl_amd import _native
    from cusrl_amd.nn.module import Linear

    torch.manual_seed(9)
    head = Linear(128, 1).to(DEV)
    x = torch.randn(4096, 128, device=DEV, requires_grad=True)
    before = _native.launch_counts.get("cusrl_narrow_linear_fwd", 0)
    with torch.no_grad():
        plain = head(x)
    out = head(x)
    assert _native.launch_counts["cusrl_narrow_linear_fwd"] == before + 2 and torch.equal(plain, out.detach())
    out.square().sum().backward()
    got = [head.weight.grad.clone(), head.bias.grad.clone(), x.grad.clone()]
    head.weight.grad = head.bias.grad = x.grad = None
    ref = torch.nn.functional.linear(x, head.weight, head.bias)
    torch.testing.assert_close(out.detach(), ref.detach(), rtol=1e-5, atol=1e-5)
    ref.square().sum().backward()
    for a, b in zip(got, [head.weight.grad, head.bias.grad, x.grad]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))


def test_narrow_head_autograd_matches_plain_linear():
    from cusrl_amd.nn.module import Linear

    torch.manual_seed(3)
    for out_features in (12, 1):
        head = Linear(128, out_features).to(DEV)
        x = torch.randn(8192, 128, device=DEV, requires_grad=True)
        head(x).square().sum().backward()
        got = [head.weight.grad.clone(), head.bias.grad.clone(), x.grad.clone()]
        head.weight.grad = head.bias.grad = x.grad = None
        torch.nn.functional.linear(x, head.weight, head.bias).square().sum().backward()
        for a, b in zip(got, [head.weight.grad, head.bias.grad, x.grad]):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))


@pytest.mark.parametrize("n", [92569, 5, 4096])
@pytest.mark.parametrize("decoupled,weight_decay,max_norm", [(False, 0.0, 1.0), (True, 0.01, None), (False, 0.01, 0.05)])
def test_adam_step_vs_oracle(ops, n, decoupled, weight_decay, max_norm):
    rng = np.random.default_rng(n)
    param = rng.standard_normal(n).astype(np.float32)
    exp_avg, exp_avg_sq, step = np.zeros(n, np.float32), np.zeros(n, np.float32), 0
    d_param, d_m, d_v = dev(param), dev(exp_avg), dev(exp_avg_sq)
    d_step, d_lr = torch.zeros(1, device=DEV), torch.full((1,), 2e-4, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(3):
        grad = (rng.standard_normal(n) * 0.02).astype(np.float32)
        d_grad = dev(grad)
        scale, norm = 1.0, None
        if max_norm is not None:
            clipped, total = oracle.clip_grad_norm(grad, max_norm)
            scale = float(min(np.float32(max_norm) / (total + np.float32(1e-6)), np.float32(1.0)))
        partials = ops.grad_sumsq(d_grad) if max_norm is not None else None
        norm = torch.zeros(1, device=DEV) if max_norm is not None else None
        ops.adam_step(d_param, d_grad, d_m, d_v, d_step, d_lr, ticket, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay,
                      decoupled=decoupled, clip_partials=partials, max_norm=max_norm, norm_out=norm)
        param, exp_avg, exp_avg_sq, step = oracle.adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=2e-4, weight_decay=weight_decay,
                                                            decoupled=decoupled, grad_scale=scale)
        if norm is not None:
            np.testing.assert_allclose(norm.item(), total, rtol=1e-6)
        assert d_step.item() == step and ticket.item() == 0
        np.testing.assert_allclose(host(d_param), param, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(host(d_m), exp_avg, rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(host(d_v), exp_avg_sq, rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_adam_step_window_pair_equals_one_launch_over_everything(ops, max_norm):
    """Round 6: the optimizer step of two windows — each its own launch, counter and ticket, both handed BOTH windows' squared-norm
    rows — leaves parameters, moments and norm bit-identical to ONE launch over the whole buffers whose rows are the two arrays in
    order (what one gradient assembly of all parameters leaves); a launch over everything keeps the second counter equal."""
    n, cut = 92_584, 46_600  # (both windows start on a 16-byte boundary)
    g = torch.Generator().manual_seed(3)
    make = lambda scale: (torch.randn(n, generator=g) * scale).to(DEV)  # noqa: E731
    joint = [make(1.0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    split = [t.clone() for t in joint]
    lr = torch.full((1,), 2e-4, device=DEV)
    step_j, step_mirror, ticket_j = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    steps = [torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)]
    tickets = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2)]
    hyper = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled=True, max_norm=max_norm)
    for _ in range(3):
        grad = make(0.02)
        rows = (ops.grad_sumsq(grad[:cut].contiguous()), ops.grad_sumsq(grad[cut:].contiguous())) if max_norm is not None else (None, None)
        norm_j, norm_s = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        ops.adam_step_window(joint[0], grad, joint[1], joint[2], step_j, lr, ticket_j, clip_partials=rows,
                             norm_out=norm_j if max_norm is not None else None, step_mirror=step_mirror, **hyper)
        for w, (lo, hi) in enumerate(((0, cut), (cut, n))):
            ops.adam_step_window(split[0][lo:hi], grad[lo:hi], split[1][lo:hi], split[2][lo:hi], steps[w], lr, tickets[w],
                                 clip_partials=rows, norm_out=norm_s if (w == 0 and max_norm is not None) else None, **hyper)
        for a, b in zip(joint, split):
            assert torch.equal(a, b)
        assert torch.equal(norm_j, norm_s) and (max_norm is None or float(norm_j) > max_norm)  # (the clip is active)
        assert step_j.item() == step_mirror.item() == steps[0].item() == steps[1].item()
        assert ticket_j.item() == tickets[0].item() == tickets[1].item() == 0
    # the rows continue each other: (a, b) sums like the one array [a | b]
    if max_norm is not None:
        single = [t.clone() for t in joint]
        step_1, ticket_1 = step_j.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
        grad = make(0.02)
        a, b = ops.grad_sumsq(grad[:cut].contiguous()), ops.grad_sumsq(grad[cut:].contiguous())
        ops.adam_step_window(joint[0], grad, joint[1], joint[2], step_j, lr, ticket_j, clip_partials=(a, b), **hyper)
        ops.adam_step(single[0], grad, single[1], single[2], step_1, lr, ticket_1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                      decoupled=True, clip_partials=torch.cat((a, b)), max_norm=max_norm)
        for x, y in zip(joint, single):
            assert torch.equal(x, y)
    # refusals of the raw entry point: rows without a first array, too many rows
    from cusrl_amd import _native

    lib = _native.lib()
    args = lambda a_ptr, na, b_ptr, nb: (joint[0].data_ptr(), grad.data_ptr(), joint[1].data_ptr(), joint[2].data_ptr(), step_j.data_ptr(),  # noqa: E731
                                         lr.data_ptr(), n, 0.9, 0.999, 1e-8, 0.0, 0, 0, a_ptr, na, b_ptr, nb, 1.0, None, None, None,
                                         ticket_j.data_ptr(), None)
    dummy = torch.zeros(4, dtype=torch.float64, device=DEV)
    assert lib.cusrl_adam_step_window(*args(None, 0, dummy.data_ptr(), 4)) == -1
    assert lib.cusrl_adam_step_window(*args(dummy.data_ptr(), 4, None, 2)) == -1
    assert lib.cusrl_adam_step_window(*args(dummy.data_ptr(), 1 << 16, dummy.data_ptr(), 1)) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,cut", [(92_584, 46_600), (5, 4), (3_000_003, 1_000_000)])
@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_adam_step_normed_measures_the_norm_it_clips_with(ops, n, cut, max_norm):
    """The step of a multi-rank job (second part of round 6): ``cusrl_adam_step_normed`` sums the squares of the whole gradient
    buffer inside the step launch (its blocks meet through the workspace) instead of a squared-norm launch in front of it.
    Against ``cusrl_grad_sumsq`` + ``cusrl_adam_step`` on the same operands: the same fp32 norm (the two routes split the fp64
    sum differently: the rounded norm may differ in its last bit once in ~1e8 draws — then the comparison loosens), hence the same
    parameters and moments to the bit; a pair of launches over two windows, side by side on two streams with a workspace each,
    equals one launch over everything; the workspace re-arms itself (odd and even launches) and survives hipGraph replays."""
    g = torch.Generator().manual_seed(n)
    make = lambda scale: (torch.randn(n, generator=g) * scale).to(DEV)  # noqa: E731
    reference = [make(1.0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    whole, split = [t.clone() for t in reference], [t.clone() for t in reference]
    lr = torch.full((1,), 2e-4, device=DEV)
    counters = lambda: (torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))  # noqa: E731
    (step_r, ticket_r), (step_w, ticket_w), (step_a, ticket_a), (step_b, ticket_b) = counters(), counters(), counters(), counters()
    work_w, work_a, work_b = ops.adam_norm_workspace(DEV), ops.adam_norm_workspace(DEV), ops.adam_norm_workspace(DEV)
    hyper = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled=True, max_norm=max_norm)
    side = torch.cuda.Stream()
    grad = make(0.02)
    norm_w, norm_s = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)

    def launches():
        ops.adam_step_normed(whole[0], grad, whole[1], whole[2], step_w, lr, ticket_w, norm_grad=grad, workspace=work_w,
                             norm_out=norm_w, **hyper)
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            ops.adam_step_normed(split[0][cut:], grad[cut:], split[1][cut:], split[2][cut:], step_b, lr, ticket_b, norm_grad=grad,
                                 workspace=work_b, **hyper)
        ops.adam_step_normed(split[0][:cut], grad[:cut], split[1][:cut], split[2][:cut], step_a, lr, ticket_a, norm_grad=grad,
                             workspace=work_a, norm_out=norm_s, **hyper)
        main.wait_stream(side)

    def check(exact_norm=None):
        norm_r = torch.zeros(1, device=DEV)
        ops.adam_step(reference[0], grad, reference[1], reference[2], step_r, lr, ticket_r, betas=(0.9, 0.999), eps=1e-8,
                      weight_decay=0.01, decoupled=True, clip_partials=ops.grad_sumsq(grad), max_norm=max_norm, norm_out=norm_r)
        torch.cuda.synchronize()
        assert torch.equal(norm_w, norm_s)  # (the grid follows the norm's buffer: every launch splits the sum alike)
        for a, b in zip(whole, split):
            assert torch.equal(a, b)
        np.testing.assert_allclose(float(norm_w), float(grad.double().square().sum().sqrt()), rtol=2e-7)
        assert max_norm is None or float(norm_w) > max_norm or n < 100
        if torch.equal(norm_w, norm_r):
            for a, b in zip(whole, reference):
                assert torch.equal(a, b)
        else:
            assert abs(float(norm_w) - float(norm_r)) <= 1.2e-7 * float(norm_r)
            for a, b in zip(whole, reference):
                torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9)
                b.copy_(a)
        assert step_r.item() == step_w.item() == step_a.item() == step_b.item()
        assert ticket_w.item() == ticket_a.item() == ticket_b.item() == 0

    for _ in range(5):  # odd and even launches: both slot sets, each re-armed by the launch in front of it
        grad.copy_(make(0.02))
        launches()
        check()
    # a NaN gradient: the norm is NaN like torch's, nothing waits forever
    if max_norm is not None and n > 100:
        poisoned = grad.clone()
        poisoned[7] = float("nan")
        probe = [t.clone() for t in whole]
        step_p, ticket_p = step_w.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
        norm_p = torch.zeros(1, device=DEV)
        ops.adam_step_normed(probe[0], poisoned, probe[1], probe[2], step_p, lr, ticket_p, norm_grad=poisoned,
                             workspace=ops.adam_norm_workspace(DEV), norm_out=norm_p, **hyper)
        assert torch.isnan(norm_p).all() and torch.isnan(probe[0]).all()
    # captured: the same three launches replayed from one hipGraph
    capture_stream = torch.cuda.Stream()
    capture_stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(capture_stream):
        with torch.cuda.graph(graph, stream=capture_stream):
            launches()
    torch.cuda.current_stream().wait_stream(capture_stream)
    for _ in range(5):
        grad.copy_(make(0.02))
        graph.replay()
        check()
    # refusals of the raw entry point
    from cusrl_amd import _native

    lib = _native.lib()
    args = lambda norm_ptr, norm_n, work: (whole[0].data_ptr(), grad.data_ptr(), whole[1].data_ptr(), whole[2].data_ptr(), step_w.data_ptr(),  # noqa: E731
                                           lr.data_ptr(), n, 0.9, 0.999, 1e-8, 0.0, 0, 0, norm_ptr, norm_n, work, 1.0, None, None, None,
                                           ticket_w.data_ptr(), None)
    assert lib.cusrl_adam_step_normed(*args(None, n, work_w.data_ptr())) == -1
    assert lib.cusrl_adam_step_normed(*args(grad.data_ptr(), 0, work_w.data_ptr())) == -1
    assert lib.cusrl_adam_step_normed(*args(grad.data_ptr(), n, None)) == -1
    assert lib.cusrl_adam_step_normed(*args(grad.data_ptr() + 4, n - 1, work_w.data_ptr())) == -3
    torch.cuda.synchronize()


def test_assemble_gradients_sums_slabs_into_slots(ops):
    rng = np.random.default_rng(3)
    shapes = [(16, 128 * 256), (1, 256), (16, 256 * 48), (1, 12), (0, 7), (3, 5), (1, 1)] * 5  # 35 pieces: two launches
    flat = torch.full((sum(n for _, n in shapes) + 3,), float("nan"), device=DEV)
    pieces, expect, offset = [], np.full(flat.numel(), np.nan, np.float32), 0
    for splits, n in shapes:
        src = rng.standard_normal((splits, n)).astype(np.float32) if splits else None
        pieces.append((None if src is None else dev(src), offset, n, splits))
        # the kernel's order: groups of four slabs (a + b) + (c + d), then the rest one by one
        total = np.zeros(n, np.float32)
        s = 0
        while splits and s + 4 <= splits:
            total = total + ((src[s] + src[s + 1]) + (src[s + 2] + src[s + 3]))
            s += 4
        for r in range(s, splits):
            total = total + src[r]
        expect[offset : offset + n] = total
        offset += n
    sumsq = ops.assemble_gradients(pieces, flat, want_sumsq=True)
    got = host(flat)
    assert np.isnan(got[offset:]).all()  # nothing written past the last slot
    np.testing.assert_array_equal(got[:offset], expect[:offset])
    # the blocks' partial sums of squares of what they wrote = the squared gradient norm the clipping needs; handed to the
    # Adam step as its clip partials they give the coefficient of clip_grad_norm_ (gradient_clipping.py:74)
    assert sumsq.dtype == torch.float64 and sumsq.numel() > 64
    np.testing.assert_allclose(float(sumsq.sum()), float((expect[:offset].astype(np.float64) ** 2).sum()), rtol=1e-6)  # fp32 squares
    n = offset - offset % 4
    param, m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step, lr, ticket = torch.zeros(1, device=DEV), torch.full((1,), 0.1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    norm = torch.zeros(1, device=DEV)
    ops.adam_step(param, flat[:n].contiguous(), m, v, step, lr, ticket, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                  decoupled=False, clip_partials=sumsq, max_norm=1.0, norm_out=norm)
    np.testing.assert_allclose(norm.item(), np.sqrt((expect[:offset].astype(np.float64) ** 2).sum()), rtol=1e-6)


@pytest.mark.parametrize("B,A,D", [(24576, 12, 1), (1000, 4, 2), (257, 32, 1), (2, 8, 1), (5000, 16, 1), (999, 20, 1),
                                   (513, 24, 1), (64, 28, 1), (70001, 12, 1)])  # last: staged reduction
@pytest.mark.parametrize("vclip", [None, 0.2])
def test_ppo_loss_std_vector_equals_repeated_matrix(ops, B, A, D, vclip):
    """A state-independent std passed as its [A] vector: same forward numbers as the repeated [B, A] matrix, d_std =
    the column sums of the matrix form's d_std."""
    rng = np.random.default_rng(B * A)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    mean, adv, ret = f(B, A), f(B, 1), f(B, D)
    vector = (rng.random(A) + 0.5).astype(np.float32)
    matrix = np.repeat(vector[None], B, 0)
    action = (mean + matrix * f(B, A)).astype(np.float32)
    curr_value, old_value = ret + 0.3 * f(B, D), ret + 0.3 * f(B, D)
    old_logp, _ = oracle.normal_logp_entropy(action, mean + 0.02 * f(B, A), matrix)
    kw = dict(clip=0.2, value_clip=vclip, w_sur=1.0, w_val=0.5, w_ent=0.01)
    args = lambda std: tuple(dev(x) for x in (adv, old_logp, action, mean, std, ret, curr_value, old_value))  # noqa: E731
    full = ops.ppo_loss_fwd_bwd(*args(matrix), **kw)
    vec = ops.ppo_loss_fwd_bwd(*args(vector), **kw)
    assert ops.ppo_loss_accepts_std_vector(A) and vec["d_std"].shape == (A,)
    for key in ("losses", "logp", "entropy", "ratio", "logp_ratio", "d_mean", "d_value"):
        assert torch.equal(vec[key], full[key]), key  # same arithmetic per element and the same reduction order
    want = full["d_std"].double().sum(0)
    torch.testing.assert_close(vec["d_std"].double(), want, rtol=1e-5, atol=1e-5 * float(full["d_std"].abs().sum(0).max()))
    assert not ops.ppo_loss_accepts_std_vector(7)


@pytest.mark.parametrize("A", [4, 12, 16, 32])
@pytest.mark.parametrize("form", ["std_vector", "std_matrix"])
def test_ppo_loss_cache_policies_change_no_bit(ops, form, A, option):
    """The objective's two shipped launch forms — default cache policy, and the [B, A] streams with the non-temporal hint (the
    footprint rule's choice beyond the Infinity Cache, forced here through ``cusrl_set_option("loss_policy", ...)``) — move the
    same bytes through the same arithmetic: every output bit-identical at a ragged batch size (a partial last block, a partial
    last wave).  (Round 5's second scalar-stream layout, measured neutral, is no longer compiled; the default form is what the
    golden / oracle tests above hold to the reference.)"""
    rng = np.random.default_rng(31 + A)
    B, D = 24576 + 37, 1
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    adv, ret = f(B, 1), f(B, D)
    curr_value, old_value = ret + 0.3 * f(B, D), ret + 0.3 * f(B, D)
    mean = f(B, A)
    vector = (rng.random(A) + 0.5).astype(np.float32)
    std = vector if form == "std_vector" else np.repeat(vector[None], B, 0)
    action = (mean + vector * f(B, A)).astype(np.float32)
    old_logp, _ = oracle.normal_logp_entropy(action, mean + 0.02 * f(B, A), np.repeat(vector[None], B, 0))
    args = tuple(dev(x) for x in (adv, old_logp, action, mean, std, ret, curr_value, old_value))
    kw = dict(clip=0.2, value_clip=0.2, w_sur=1.0, w_val=0.5, w_ent=0.01)
    results = {}
    for policy in (1, 2):
        option("loss_policy", policy)
        results[policy] = ops.ppo_loss_fwd_bwd(*args, **kw)
    for name in ("logp", "entropy", "ratio", "logp_ratio", "d_mean", "d_value", "d_std", "losses"):
        assert torch.equal(results[2][name], results[1][name]), name


def test_options_are_validated_and_readable(ops):
    from cusrl_amd import _native

    lib = _native.lib()
    assert lib.cusrl_set_option(b"no_such_option", 1) == -1 and lib.cusrl_set_option(None, 1) == -1
    assert lib.cusrl_set_option(b"gae_block", 100) == -3 and lib.cusrl_set_option(b"loss_policy", 3) == -3
    assert lib.cusrl_set_option(b"gru_bias_rows", 5) == -3 and lib.cusrl_set_option(b"colsum_rows", 2) == -3
    for key, value in (("gae_policy", 6), ("gae_block", 128), ("loss_policy", 2), ("push_policy", 1), ("colsum_rows", 32),
                       ("head_rows", 64), ("gru_bias_rows", 8)):
        _native.set_option(key, value)
        assert _native.get_option(key) == value
        _native.set_option(key, 0)
        assert _native.get_option(key) == 0


@pytest.mark.parametrize("form", ["std_vector", "std_matrix", "categorical", "value_only"])
def test_ppo_loss_deferred_finalize_accumulates_block_rows(ops, form):
    """CUSRL_LOSS_DEFER (what a captured minibatch step runs): one launch, no finalize.  Two launches add their block sums
    into the caller's rows — drained, they are the two launches' losses and metric means; the per-sample outputs and
    gradients are bit-identical to the two-launch form; a std vector's d_std arrives as the blocks' column sums, which
    ``assemble_gradients`` reduces to the same vector.  The value term's own launch: two launches leave exactly twice one
    launch's block rows (doubling is exact), d_value is the non-deferred call's."""
    rng = np.random.default_rng(7)
    B, A, D = 24576, 12, 1
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    adv, ret = f(B, 1), f(B, D)
    curr_value = ret + 0.3 * f(B, D)
    kw = dict(clip=0.2, value_clip=None, w_sur=1.0, w_val=0.5, w_ent=0.01)
    if form == "value_only":
        old_value = ret + 0.3 * f(B, D)
        for vclip in (None, 0.2):
            value_args = (dev(ret), dev(curr_value), dev(old_value))
            plain = ops.value_loss_fwd_bwd(*value_args, value_clip=vclip, w_val=0.5)
            rows = ops.DeferredLoss(B, A, D, torch.device(DEV), categorical=False)
            assert rows.value_rows.shape == (24, 2)  # 1024 elements per block
            first = ops.value_loss_fwd_bwd(*value_args, value_clip=vclip, w_val=0.5, deferred=rows)
            once = rows.value_rows.clone()
            second = ops.value_loss_fwd_bwd(*value_args, value_clip=vclip, w_val=0.5, deferred=rows)
            assert "losses" not in first and float(once.abs().sum()) > 0.0
            assert torch.equal(rows.value_rows, 2 * once)
            assert torch.equal(first["d_value"], plain["d_value"]) and torch.equal(second["d_value"], plain["d_value"])
            sums = host(once).sum(0)  # the finalize launch's inputs, added up in another order: fp32 rounding of `losses`
            np.testing.assert_allclose(sums[0] / (B * D) * 0.5, host(plain["losses"])[0], rtol=2e-7, atol=1e-12)
            np.testing.assert_allclose(sums[1] / B, host(plain["losses"])[1], rtol=2e-7, atol=1e-9)
        return
    if form == "categorical":
        logits = 2.0 * f(B, A)
        action = np.eye(A, dtype=np.float32)[rng.integers(0, A, B)]
        old_logp = oracle.categorical_ppo_loss(adv, np.zeros((B, 1), np.float32), action, logits + 0.05 * f(B, A), ret, curr_value)["logp"]
        args = tuple(dev(x) for x in (adv, old_logp, action, logits, ret, curr_value)) + (None,)
        call, grads = ops.ppo_loss_categorical_fwd_bwd, ("d_logits", "d_value")
    else:
        mean = f(B, A)
        vector = (rng.random(A) + 0.5).astype(np.float32)
        std = vector if form == "std_vector" else np.repeat(vector[None], B, 0)
        action = (mean + vector * f(B, A)).astype(np.float32)
        old_logp, _ = oracle.normal_logp_entropy(action, mean + 0.02 * f(B, A), np.repeat(vector[None], B, 0))
        args = tuple(dev(x) for x in (adv, old_logp, action, mean, std, ret, curr_value)) + (None,)
        call, grads = ops.ppo_loss_fwd_bwd, ("d_mean", "d_value") + (("d_std",) if form == "std_matrix" else ())
    plain = call(*args, **kw)
    rows = ops.DeferredLoss(B, A, D, torch.device(DEV), categorical=form == "categorical")
    assert rows.blocks == (96 if form == "categorical" else 98) and rows.drain(1) is None  # nothing recorded yet
    first = call(*args, deferred=rows, **kw)
    second = call(*args, deferred=rows, **kw)
    assert "losses" not in first
    for key in ("logp", "entropy", "ratio", "logp_ratio") + grads:
        assert torch.equal(first[key], plain[key]) and torch.equal(second[key], plain[key]), key
    drained = rows.drain(2)
    losses = host(plain["losses"]).astype(np.float64)
    for name, index in (("value_loss", 0), ("surrogate_loss", 1), ("entropy_loss", 2), ("ratio", 3), ("entropy", 4), ("value", 5)):
        total, count = drained[name]
        assert count == (1 if index < 3 else B)
        np.testing.assert_allclose(total / 2, losses[index], rtol=2e-7, atol=1e-12, err_msg=name)  # fp32 rounding of `losses`
    assert float(rows.rows.abs().sum()) == 0.0  # drained rows start over
    if form == "std_vector":
        columns = first["d_std"]
        assert isinstance(columns, ops.DeferredColumns) and columns.splits == 98 and columns.numel == A
        torch.testing.assert_close(columns.materialize(), plain["d_std"], rtol=1e-5, atol=1e-9)
        flat = torch.full((A + 4,), float("nan"), device=DEV)
        ops.assemble_gradients([(columns, 4, A, columns.splits)], flat)
        torch.testing.assert_close(flat[4:], plain["d_std"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("B,A,D", [(24576, 12, 1), (1000, 7, 1), (513, 32, 2), (3, 40, 1), (255, 4, 3), (70001, 12, 1)])
@pytest.mark.parametrize("vclip", [None, 0.2])
@pytest.mark.parametrize("form", ["std_matrix", "std_vector", "categorical"])
def test_value_term_alone_plus_policy_terms_equal_the_one_launch_objective(ops, B, A, D, vclip, form):
    """Round 6: inside a captured step with the critic on its own stream the value term is ONE launch there
    (``cusrl_value_loss_fwd_bwd``) and the surrogate + entropy terms another on the actor's stream (``D = 0`` form of
    ``cusrl_ppo_loss_fwd_bwd``).  Together they must be the one-launch objective: d_value, d_mean / d_logits, d_std and every
    per-sample output BIT-identical (same per-element arithmetic), the three losses and the metric means to fp32 rounding of
    a different summation order — and against the oracle (value.py:85-89,121-137)."""
    if form == "std_vector" and not ops.ppo_loss_accepts_std_vector(A):
        pytest.skip("the std-vector form exists for action widths that are a multiple of 4 up to 32")
    rng = np.random.default_rng(B + A + D)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    adv, ret = f(B, 1), f(B, D)
    curr_value, old_value = ret + 0.3 * f(B, D), ret + 0.3 * f(B, D)
    kw = dict(clip=0.2, value_clip=vclip, w_sur=1.0, w_val=0.5, w_ent=0.01)
    if form == "categorical":
        logits = 2.0 * f(B, A)
        action = np.eye(A, dtype=np.float32)[rng.integers(0, A, B)]
        old_logp = oracle.categorical_ppo_loss(adv, np.zeros((B, 1), np.float32), action, logits + 0.05 * f(B, A), ret, curr_value)["logp"]
        head = tuple(dev(x) for x in (adv, old_logp, action, logits))
        call, grads = ops.ppo_loss_categorical_fwd_bwd, ("d_logits",)
    else:
        mean = f(B, A)
        vector = (rng.random(A) + 0.5).astype(np.float32)
        std = vector if form == "std_vector" else np.repeat(vector[None], B, 0)
        action = (mean + vector * f(B, A)).astype(np.float32)
        old_logp, _ = oracle.normal_logp_entropy(action, mean + 0.02 * f(B, A), np.repeat(vector[None], B, 0))
        head = tuple(dev(x) for x in (adv, old_logp, action, mean, std))
        call, grads = ops.ppo_loss_fwd_bwd, ("d_mean", "d_std")
    value_args = tuple(dev(x) for x in (ret, curr_value, old_value))
    whole = call(*head, *value_args, **kw)
    policy = call(*head, None, None, None, **kw)
    value = ops.value_loss_fwd_bwd(*value_args, value_clip=vclip, w_val=0.5)
    assert "d_value" not in policy
    assert torch.equal(value["d_value"], whole["d_value"])
    for key in ("logp", "entropy", "logp_ratio", "ratio") + grads:
        assert torch.equal(policy[key], whole[key]), key
    w, p, v = host(whole["losses"]), host(policy["losses"]), host(value["losses"])
    assert p[0] == 0.0 and p[5] == 0.0 and p[6] == np.float32(p[1] + p[2])
    np.testing.assert_array_equal(p[1:5], w[1:5])
    np.testing.assert_allclose(v[0], w[0], rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(v[1], w[5], rtol=2e-6, atol=1e-7)
    err = curr_value.astype(np.float64) - ret
    if vclip is None:
        want = (err ** 2).mean() * 0.5
    else:
        clipped = old_value.astype(np.float64) + np.clip(curr_value.astype(np.float64) - old_value, -vclip, vclip)
        want = np.maximum(err ** 2, (clipped - ret) ** 2).mean() * 0.5
    np.testing.assert_allclose(v[0], want, rtol=1e-5)
    # the deferred-finalize forms of both launches: their sums land in separate rows and drain to the same six metrics
    rows = ops.DeferredLoss(B, A, D, torch.device(DEV), categorical=form == "categorical")
    for _ in range(2):
        deferred_policy = call(*head, None, None, None, deferred=rows, **kw)
        deferred_value = ops.value_loss_fwd_bwd(*value_args, value_clip=vclip, w_val=0.5, deferred=rows)
    assert "losses" not in deferred_value and torch.equal(deferred_value["d_value"], whole["d_value"])
    drained = rows.drain(2)
    for name, index in (("value_loss", 0), ("surrogate_loss", 1), ("entropy_loss", 2), ("ratio", 3), ("entropy", 4), ("value", 5)):
        total, count = drained[name]
        assert count == (1 if index < 3 else B)
        np.testing.assert_allclose(total / 2, w[index], rtol=2e-6, atol=1e-7, err_msg=name)
    assert float(rows.rows.abs().sum()) == 0.0 and float(rows.value_rows.abs().sum()) == 0.0
    if form == "std_vector":
        torch.testing.assert_close(deferred_policy["d_std"].materialize(), whole["d_std"], rtol=1e-5, atol=1e-9)


def test_value_term_argument_errors(ops):
    from cusrl_amd import _native

    lib = _native.lib()
    x = torch.zeros(8, 1, device=DEV)
    rows = torch.zeros(1, 2, dtype=torch.float64, device=DEV)
    out = torch.zeros(2, device=DEV)
    assert lib.cusrl_value_loss_fwd_bwd(x.data_ptr(), x.data_ptr(), None, 8, 1, 0.2, 0.5, out.data_ptr(), None, rows.data_ptr(), 0, None) == -1
    assert lib.cusrl_value_loss_fwd_bwd(x.data_ptr(), x.data_ptr(), None, 0, 1, -1.0, 0.5, out.data_ptr(), None, rows.data_ptr(), 0, None) == -1
    assert lib.cusrl_value_loss_fwd_bwd(x.data_ptr(), x.data_ptr(), None, 8, 1, -1.0, 0.5, None, None, rows.data_ptr(), 0, None) == -1
    assert lib.cusrl_value_loss_blocks(24576, 1) == 24 and lib.cusrl_value_loss_blocks(0, 1) == 0


@pytest.mark.parametrize("B,A,D", [(98304, 12, 1), (1000, 7, 1), (3, 40, 2), (257, 4, 3)])
def test_policy_stats_vs_oracle(ops, B, A, D):
    rng = np.random.default_rng(B + A + D)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    mp, sp = f(B, A), (rng.random((B, A)) + 0.5).astype(np.float32)
    mq, sq = mp + 0.05 * f(B, A), (sp * np.exp(0.05 * f(B, A))).astype(np.float32)  # an updated policy: close to the old
    action = (mp + sp * f(B, A)).astype(np.float32)
    old_logp, _ = oracle.normal_logp_entropy(action, mp, sp)
    advantage = f(B, D)
    got = host(ops.policy_stats(*(dev(x) for x in (mp, sp, mq, sq, action, old_logp, advantage))))
    want = oracle.policy_stats(mp, sp, mq, sq, action, old_logp, advantage)
    # the KL of two close Gaussians cancels to ~1e-3 of its terms: absolute fp32 error of the per-element terms
    np.testing.assert_allclose(got[0], want[0], rtol=1e-4, atol=2e-7 * A)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-6)


def test_assign_rows_equals_index_put(ops):
    torch.manual_seed(0)
    for shape, dtype in (((4096, 48), torch.float32), ((100, 7), torch.float32), ((64, 3, 5), torch.float32), ((33, 1), torch.bool)):
        dst = (torch.rand(shape, device=DEV) > 0.5) if dtype == torch.bool else torch.randn(shape, device=DEV)
        indices = torch.randperm(shape[0], device=DEV)[: max(shape[0] // 7, 1)].sort().values
        src = (torch.rand((indices.numel(),) + shape[1:], device=DEV) > 0.5) if dtype == torch.bool else torch.randn(
            (indices.numel(),) + shape[1:], device=DEV)
        want = dst.clone()
        want[indices] = src
        ops.assign_rows(dst, indices, src)
        assert torch.equal(dst, want)
    ops.assign_rows(dst, indices[:0], src[:0])  # empty: no launch


def test_scatter_rows_with_a_device_count_at_every_lane_unit(ops):
    """``scatter_rows`` under a count the kernel reads, with ``uint8`` rows so that the row size alone picks the lane unit
    (16 / 8 / 4 / 2 / 1 bytes), over two blocks, and from a source that is only 4-byte aligned; then ``splice_rows`` with
    an ``init`` that is only 8-byte aligned.  Bit-exact against ``index_put`` on a sentinel-filled destination."""
    generator = torch.Generator(device=DEV).manual_seed(11)
    sentinel = 0xA5  # the source bytes stay below 128: a row that still holds the sentinel was not written
    for K, W, skew in ((40, 48, 0), (40, 24, 0), (40, 12, 0), (40, 6, 0), (40, 3, 0), (70, 256, 0), (40, 48, 4)):
        rows = 64 if K <= 64 else 128
        base = torch.randint(0, 128, (K * W + skew,), dtype=torch.uint8, device=DEV, generator=generator)
        src = base[skew:].view(K, W)
        assert src.is_contiguous() and src.data_ptr() % 16 == skew
        indices = torch.randperm(rows, device=DEV, generator=generator)[:K]  # unique rows: no dependence on store order
        for count in (0, 3, K, K + 5):
            dst = torch.full((rows, W), sentinel, dtype=torch.uint8, device=DEV)
            want = dst.clone()
            want[indices[: min(K, count)]] = src[: min(K, count)]
            ops.scatter_rows(src, indices, dst, torch.tensor([count], dtype=torch.int32, device=DEV))
            assert torch.equal(dst, want), (K, W, skew, count)
    N, W = 33, 48
    src = torch.randint(0, 128, (N, W), dtype=torch.uint8, device=DEV, generator=generator)
    init = torch.randint(0, 128, (N * W + 8,), dtype=torch.uint8, device=DEV, generator=generator)[8:].view(N, W)
    assert init.data_ptr() % 16 == 8 and src.data_ptr() % 16 == 0
    done = torch.rand(N, 1, device=DEV, generator=generator) < 0.3
    finished = done.squeeze(-1).nonzero().squeeze(-1)
    indices = torch.zeros(N, dtype=torch.int64, device=DEV)
    indices[: finished.numel()] = finished
    count = torch.tensor([finished.numel()], dtype=torch.int32, device=DEV)
    dst = torch.full_like(src, sentinel)
    ops.splice_rows(src, init, indices, count, done, dst)
    expect = src.clone()
    expect[finished] = init[: finished.numel()]
    assert torch.equal(dst, expect)


def test_gather_two_byte_unit_leaves_bit_exact(ops):
    """``float16`` leaves of 3 and of 1 channel: 6- and 2-byte rows, the gather's 2-byte lane unit (no other case takes it)."""
    T, N, B = 3, 5, 7
    rng = np.random.default_rng(T * N + B)
    leaves = [rng.standard_normal((T, N, 3)).astype(np.float16), rng.standard_normal((T, N, 1)).astype(np.float16)]
    idx = rng.permutation(T * N)[:B].astype(np.int64)
    for x, out in zip(leaves, ops.gather_rows([dev(x) for x in leaves], dev(idx), T, N)):
        assert np.array_equal(host(out), oracle.gather_rows(x, idx)), x.shape
    env_idx = rng.permutation(N)[:3].astype(np.int64)
    for x, out in zip(leaves, ops.gather_rows([dev(x) for x in leaves], dev(env_idx), T, N, temporal=True)):
        assert np.array_equal(host(out), oracle.gather_rows(x, env_idx, temporal=True)), x.shape


def test_assemble_gradients_reduces_deferred_column_windows(ops):
    """Partial rows of the column-sum kernels: a window [column, column + numel) of rows of width row_stride."""
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((384, 1680)).astype(np.float32)
    few = rng.standard_normal((5, 40)).astype(np.float32)
    d_rows, d_few = dev(rows), dev(few)
    flat = torch.full((1536 + 12 + 128 + 40 + 7,), float("nan"), device=DEV)
    pieces = [(ops.DeferredColumns(d_rows, 384, 1680, 0, 1536), 0, 1536, 0),
              (ops.DeferredColumns(d_rows, 384, 1680, 1664, 12), 1536, 12, 0),
              (ops.DeferredColumns(d_rows, 384, 1680, 1536, 128), 1548, 128, 0),
              (ops.DeferredColumns(d_few, 5, 40, 0, 40), 1676, 40, 0),   # few rows: the per-element path with a stride
              (None, 1716, 7, 0)]
    ops.assemble_gradients(pieces, flat)
    got = host(flat).astype(np.float64)
    want = np.concatenate([rows[:, :1536].sum(0, dtype=np.float64), rows[:, 1664:1676].sum(0, dtype=np.float64),
                           rows[:, 1536:1664].sum(0, dtype=np.float64), few.sum(0, dtype=np.float64), np.zeros(7)])
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(rows).sum(0).max())
    torch.testing.assert_close(pieces[1][0].materialize().double(), torch.from_numpy(want[1536:1548]).to(DEV), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("rows,K,H", [(24576, 48, 256), (1000, 12, 64), (37, 60, 128), (4097, 4, 320), (8, 48, 256), (98304, 48, 256)])
@pytest.mark.parametrize("mask", [True, False])
def test_input_layer_backward_matches_float64(ops, rows, K, H, mask, gradient_parity):
    """``cusrl_input_layer_bwd`` (round 6): ReLU mask + bias gradient + weight gradient of the bottom layer from ONE pass,
    against float64 ``(g * (y > 0)).T @ x`` / ``.sum(0)`` (what autograd's threshold_backward, sum and mm compute,
    cusrl/nn/module/mlp.py:89-90) to 1e-5 of each gradient's largest entry; a second launch is bit-identical."""
    torch.manual_seed(rows + K + H)
    g = torch.randn(rows, H, device=DEV)
    y = torch.relu(torch.randn(rows, H, device=DEV)) if mask else None
    x = torch.randn(rows, K, device=DEV)
    weight = torch.empty(H, K, device=DEV)
    assert ops.input_layer_supported(g, y, x, weight)
    first = ops.input_layer_backward(g, y, x)
    second = ops.input_layer_backward(g, y, x)
    masked = (g * (y > 0) if mask else g).double()
    want_w, want_b = masked.t() @ x.double(), masked.sum(0)
    assert first[0].shape == (H, K) and first[1].shape == (H,)
    gradient_parity(f"input_layer.dW[{rows},{K},{H},{mask}]", host(first[0]), host(want_w), 1e-5)
    # a bias gradient is a sum of `rows` signed terms that cancel: its yardstick is the sum of their magnitudes per column
    scale = float(masked.abs().sum(0).max())
    assert float((first[1].double() - want_b).abs().max()) <= 1e-6 * scale
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])  # fixed summation order


def test_input_layer_argument_errors(ops):
    from cusrl_amd import _native

    lib = _native.lib()
    assert not lib.cusrl_input_layer_supported(50, 256) and not lib.cusrl_input_layer_supported(64, 256)
    assert not lib.cusrl_input_layer_supported(48, 100) and lib.cusrl_input_layer_supported(48, 256)
    g, x = torch.zeros(8, 256, device=DEV), torch.zeros(8, 48, device=DEV)
    ws = torch.zeros(16, 256 * 49, device=DEV)
    call = lambda *a: lib.cusrl_input_layer_bwd(*a, None)  # noqa: E731
    assert call(None, None, x.data_ptr(), 8, 48, 256, ws.data_ptr(), ws.data_ptr()) == -1
    assert call(g.data_ptr(), None, x.data_ptr(), 0, 48, 256, ws.data_ptr(), ws.data_ptr()) == -1
    assert call(g.data_ptr(), None, x.data_ptr(), 8, 50, 256, ws.data_ptr(), ws.data_ptr()) == -3
    assert call(g.data_ptr() + 4, None, x.data_ptr(), 8, 48, 256, ws.data_ptr(), ws.data_ptr()) == -3
    assert lib.cusrl_input_layer_row_blocks(24576, 256) == 64 and lib.cusrl_input_layer_row_blocks(0, 256) == 0


def test_flat_backward_with_deferred_sums_matches_plain_autograd():
    """The agent's backward: split-GEMM slabs, deferred bias / head column sums, all summed by the assembly launch."""
    from cusrl_amd.nn.module import Linear, Mlp, collect_split_weight_grads
    from cusrl_amd.utils.distributed import FlatGradients

    torch.manual_seed(11)
    mlp = Mlp(48, (256, 128), ends_with_activation=True).to(DEV)
    head = Linear(128, 12).to(DEV)
    value_mlp = Mlp(48, (256, 128), ends_with_activation=True).to(DEV)
    value_head = Linear(128, 1).to(DEV)
    modules = torch.nn.ModuleList([mlp, head, value_mlp, value_head])
    optimizer = torch.optim.SGD(modules.parameters(), lr=0.1)
    flat = FlatGradients(optimizer)
    x = torch.randn(8192, 48, device=DEV)

    def loss_of(layers_only):
        a = (_plain_layers(mlp, x) if layers_only else mlp(x))
        b = (_plain_layers(value_mlp, x) if layers_only else value_mlp(x))
        pa = torch.nn.functional.linear(a, head.weight, head.bias) if layers_only else head(a)
        pb = torch.nn.functional.linear(b, value_head.weight, value_head.bias) if layers_only else value_head(b)
        return pa.square().mean() + pb.square().mean()

    with collect_split_weight_grads() as sink:
        grads = torch.autograd.grad(loss_of(False), flat.params, allow_unused=True)
    # every gradient took the deferred route — but the two bottom layers' (round 6: their weight and bias gradients come
    # finished out of cusrl_input_layer_bwd)
    assert sum(g is None for g in grads) == len(flat.params) - 4
    assert all(g is not None for g, p in zip(grads, flat.params) if p.shape in ((256, 48), (256,)))
    flat.assemble(grads, sink)
    want = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss_of(True), flat.params)])
    torch.testing.assert_close(flat.packed(), want, rtol=2e-4, atol=1e-4 * float(want.abs().max()))


def test_fused_linear_paths_match_plain_autograd():
    from cusrl_amd.nn.module import Mlp

    torch.manual_seed(0)
    for rows in (64, 8192):
        mlp = Mlp(48, (256, 128), ends_with_activation=True).to(DEV)
        x = torch.randn(rows, 48, device=DEV, requires_grad=True)
        mlp(x).square().sum().backward()
        got = [p.grad.clone() for p in mlp.parameters()] + [x.grad.clone()]
        for p in mlp.parameters():
            p.grad = None
        x.grad = None
        _plain_layers(mlp, x).square().sum().backward()  # torch's own ops: addmm, relu, autograd backward
        want = [p.grad for p in mlp.parameters()] + [x.grad]
        for g, w in zip(got, want):
            torch.testing.assert_close(g, w, rtol=2e-4, atol=1e-4 * float(w.abs().max()))
        with torch.no_grad():
            assert torch.equal(mlp(x), mlp.layers(x))


def test_side_stream_runs_beside_the_stream_it_was_made_for():
    """Second part of round 6: a side stream is chosen by demonstration — work issued to it makes progress while the stream it has
    to overlap with is busy (HIP maps streams onto a few hardware queues; two streams of one queue run serially, and which queue
    a new stream gets depends on how many the process created before: the draw-ahead stream of a torchrun rank shared the main
    stream's).  A stream trivially does not run beside itself."""
    from cusrl_amd.utils.streams import runs_beside, side_stream

    main = torch.cuda.current_stream()
    for _ in range(6):  # whatever the process has created so far
        stream = side_stream(DEV)
        assert stream != main and runs_beside(stream, [main])
    assert not runs_beside(main, [main])
    other = side_stream(DEV, beside=[main, stream])
    assert runs_beside(other, [main, stream])


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("rows,D", [(98304, 1), (1001, 1), (4099, 3)])
def test_normalize_from_gathered_equals_merge_then_normalize(ops, W, rows, D):
    """Second part of round 6: the advantage normalisation of a multi-rank job — ``cusrl_normalize_from_gathered`` (merge of the
    all-gathered ``mean | var`` rows + normalisation, one launch) against ``cusrl_merge_mean_var`` + ``cusrl_normalize``: the same
    operations in the same order, bit for bit; the row it gathers is the two halves of ``adv_stats_finalize``'s result as they are."""
    g = torch.Generator().manual_seed(rows + W)
    x = (torch.randn(rows, D, generator=g) * 3 + 0.5).to(DEV)
    var, mean = ops.adv_stats_finalize(ops.col_stats(x), rows)
    row = ops.packed_mean_var(mean, var)
    assert row.data_ptr() == mean.data_ptr() and row.shape == (2 * D,) and torch.equal(row, torch.cat((mean, var)))
    assert torch.equal(ops.packed_mean_var(mean.clone(), var), torch.cat((mean, var)))  # (anything else: a cat)
    others = [(row + 0.1 * torch.randn(2 * D, generator=g).to(DEV)).abs() for _ in range(W - 1)]
    gathered = torch.stack([row] + others)
    expect, merged_mean, merged_var = x.clone(), torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    ops.merge_mean_var(gathered, merged_mean, merged_var)
    ops.normalize_(expect, merged_mean, merged_var, 1e-8)
    got = x.clone()
    got_var, got_mean = ops.normalize_from_gathered_(got, gathered, 1e-8)
    assert torch.equal(got, expect) and torch.equal(got_mean, merged_mean) and torch.equal(got_var, merged_var)
    if W == 1:  # one rank: the merge is the identity — the single-process launch's result
        single = x.clone()
        ops.normalize_from_partials_(single, ops.col_stats(x), rows, 1e-8)
        assert torch.equal(got, single)
