"""Shared cases of the batched device map operations (xe_map_lookup_batch_device / _update_ / _delete_):
tests/test_mapops.py runs them on the host simulation, tests/test_mapops_gpu.py on the product library.

Every expected value comes from an oracle VM (oracle/liboracle.so) given the same operations through its
single-key map_update / map_lookup / map_delete, in batch order; map_dump (sorted by key) and map_count
are compared after every step. VMs run the shared interpreter (engine=1): nothing compiles.

`dev` turns a numpy array into what the VM methods take for device memory: the array itself on the host
simulation (device addresses are host addresses there), a CUDA tensor on the product."""
from __future__ import annotations

import numpy as np

from gobpfld_amd import workloads as W
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, VM,
                                  EmulatorError, MapDef, Settings)

ERR_INVAL, ERR_NOMEM, ERR_UNSUPPORTED = -22, -12, -95
KEY_SIZES = (4, 8, 13, 64)
VALUE_SIZES = (1, 8, 24, 4096)
# 70,001: more than the 65,536 entries that one pass of the kernels' grid covers at one entry per lane
# (256 workgroups x 256 lanes before the lanes start to stride, xe_mapops.hip), and no multiple of a wave,
# a workgroup or a value sub-group
COUNTS = (0, 1, 63, 64, 65, 70001)
HASH_MAX, ARRAY_MAX, HASH_CAP = 64, 100, 128
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- xe_hash_words, restated
def hash_words(key: bytes) -> int:
    """xe_internal.h xe_hash_words over the zero-padded little-endian key words."""
    ks = len(key)
    padded = key + b"\0" * (-ks % 8)
    h = 0x9E3779B97F4A7C15 ^ ((ks * 0xC2B2AE3D27D4EB4F) & M64)
    for i in range(0, len(padded), 8):
        h ^= int.from_bytes(padded[i:i + 8], "little")
        h = (h * 0xff51afd7ed558ccd) & M64
        h ^= h >> 32
    h ^= h >> 29
    h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 32
    return h


def home_slot(key: bytes, cap: int = HASH_CAP) -> int:
    return hash_words(key) & 0xffffffff & (cap - 1)


def keys_with_home(ks: int, want, count: int, start: int = 0) -> list[bytes]:
    """The first `count` keys (a counter in the key's leading bytes) whose home slot is in `want`."""
    out, i = [], start
    while len(out) < count:
        k = i.to_bytes(8, "little")[:ks].ljust(ks, b"\x5a")
        if home_slot(k) in want:
            out.append(k)
        i += 1
    return out


def rwords(ks: int) -> int:
    r = 1
    while r < 1 + (ks + 7) // 8:
        r <<= 1
    return r


def guard_hash_restatement(lib, ks: int = 8) -> None:
    """One key into an empty map, the state exported: the one occupied record sits at hash & (cap - 1)."""
    vm = VM(Settings(engine=1), lib=lib)
    vs = 8
    m = vm.add_map(MapDef(MAP_HASH, ks, vs, HASH_MAX))
    for key in (b"\x01" * ks, bytes(range(ks)), (12345).to_bytes(8, "little")[:ks].ljust(ks, b"\x77")):
        vm.map_update(m, key, b"\x11" * vs)
        nbytes = vm.map_state_bytes(m)
        img = np.zeros(nbytes, dtype=np.uint8)
        vm.map_state_export(m, img.ctypes.data)
        vals_alloc = max(8, ((HASH_CAP + 1) * vs + 7) & ~7)
        rec = img[vals_alloc:vals_alloc + (HASH_CAP + 1) * rwords(ks) * 8].view(np.uint64).reshape(HASH_CAP + 1, rwords(ks))
        full = np.nonzero(rec[:, 0] & np.uint64(1))[0]
        assert list(full) == [home_slot(key)], (key, list(full), home_slot(key))
        vm.map_delete(m, key)
    vm.close()


# ---------------------------------------------------------------- oracle comparison
def same_map(vm: VM, ref: VM, m: int, what: str) -> None:
    got, want = vm.map_dump(m), ref.map_dump(m)
    if isinstance(want, tuple):
        assert np.array_equal(got[0], want[0]), f"{what}: keys differ"
        assert np.array_equal(got[1], want[1]), f"{what}: values differ"
        assert vm.map_count(m) == ref.map_count(m), f"{what}: count differs"
    else:
        assert got == want, f"{what}: values differ"


def ref_update(ref: VM, m: int, keys: np.ndarray, vals: np.ndarray) -> None:
    for k, v in zip(keys, vals):
        ref.map_update(m, k.tobytes(), v.tobytes())


def ref_lookup(ref: VM, m: int, keys: np.ndarray, vs: int):
    """(values, found) of the oracle's single-key lookups; one call per distinct key."""
    memo: dict[bytes, bytes | None] = {}
    vals = np.zeros((len(keys), vs), dtype=np.uint8)
    found = np.zeros(len(keys), dtype=np.uint8)
    for i, k in enumerate(keys):
        kb = k.tobytes()
        if kb not in memo:
            try:
                memo[kb] = ref.map_lookup(m, kb)
            except EmulatorError:  # (an ARRAY index out of range: the reference reports an error; absent here)
                memo[kb] = None
        if memo[kb] is not None:
            vals[i] = np.frombuffer(memo[kb], dtype=np.uint8)
            found[i] = 1
    return vals, found


def ref_delete(ref: VM, m: int, keys: np.ndarray) -> None:
    for k in keys:
        ref.map_delete(m, k.tobytes())


def to_np(x) -> np.ndarray:
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def check_lookup(vm: VM, ref: VM, m: int, keys: np.ndarray, vs: int, dev, what: str) -> None:
    vals, found = vm.map_lookup_batch(m, dev(keys))
    wv, wf = ref_lookup(ref, m, keys, vs)
    assert np.array_equal(to_np(found), wf), f"{what}: found differs"
    assert np.array_equal(to_np(vals), wv), f"{what}: values differ"


def pair(lib, oracle_lib, mdef: MapDef):
    vm, ref = VM(Settings(engine=1), lib=lib), VM(Settings(engine=1), lib=oracle_lib)
    return vm, ref, vm.add_map(mdef), ref.add_map(mdef)


def hash_pool(rng, ks: int, n: int) -> np.ndarray:
    """n distinct random keys of ks bytes."""
    pool = rng.integers(0, 256, size=(4 * n, ks), dtype=np.uint8)
    pool = np.unique(pool, axis=0)
    rng.shuffle(pool)
    assert len(pool) >= n
    return np.ascontiguousarray(pool[:n])


# ---------------------------------------------------------------- 1. matrix
def run_matrix(lib, oracle_lib, dev, kind: int, ks: int, vs: int) -> None:
    rng = np.random.default_rng(1000 * ks + vs + kind)
    array = kind == MAP_ARRAY
    vm, ref, m, rm = pair(lib, oracle_lib, MapDef(kind, 4 if array else ks, vs, ARRAY_MAX if array else HASH_MAX))
    assert m == rm
    if array:
        pool = np.arange(ARRAY_MAX, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
        absent = np.array([ARRAY_MAX, ARRAY_MAX + 7, 0xffffffff], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    else:
        both = hash_pool(rng, ks, HASH_MAX + 16)
        pool, absent = both[:HASH_MAX], both[HASH_MAX:]
    for n in COUNTS:
        # up to the pool's size: distinct keys in a random order; one more: a repeated key; 70,001: draws
        # from the pool (every key many times: the last value of each wins)
        pick = rng.permutation(len(pool))[:n] if n <= len(pool) else rng.integers(0, len(pool), size=n)
        if n == 65:
            pick = np.concatenate([rng.permutation(HASH_MAX), [int(rng.integers(0, HASH_MAX))]])
        keys = np.ascontiguousarray(pool[pick])
        vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
        vm.map_update_batch_device(m, dev(keys), dev(vals))
        ref_update(ref, m, keys, vals)
        same_map(vm, ref, m, f"update of {n}")
        probe = np.ascontiguousarray(np.concatenate([keys[: min(n, 300)], absent, pool[:5]]))
        check_lookup(vm, ref, m, probe, vs, dev, f"lookup after the update of {n}")
        if n == COUNTS[-1]:
            check_lookup(vm, ref, m, keys, vs, dev, f"lookup of {n}")
        if array:
            continue
        # delete a third of what was written (repetitions kept) and a few absent keys
        dk = np.ascontiguousarray(np.concatenate([keys[::3], absent[:3]]))
        _, present = ref_lookup(ref, m, dk, vs)
        found = vm.map_delete_batch(m, dev(dk))
        assert np.array_equal(to_np(found), present), f"delete after the update of {n}: found differs"
        ref_delete(ref, m, dk)
        check_lookup(vm, ref, m, probe, vs, dev, f"lookup after the delete ({n})")
        same_map(vm, ref, m, f"delete after the update of {n}")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. probe chains
def run_probe_chains(lib, oracle_lib, dev, ks: int = 8, vs: int = 24) -> None:
    rng = np.random.default_rng(7)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, HASH_MAX))
    # >= 20 keys whose home is one of the last four slots of the 128-slot table: the chain wraps to slot 0
    wrap = keys_with_home(ks, range(HASH_CAP - 4, HASH_CAP), 24)
    assert len(set(wrap)) == 24 and all(home_slot(k) >= HASH_CAP - 4 for k in wrap)
    keys = np.frombuffer(b"".join(wrap), dtype=np.uint8).reshape(-1, ks)
    vals = rng.integers(0, 256, size=(len(keys), vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    ref_update(ref, m, keys, vals)
    check_lookup(vm, ref, m, keys, vs, dev, "wrapping chain")
    # ten keys of one home slot, away from the wrapped chain; the third is deleted: the chain is cut in the middle
    chain = keys_with_home(ks, (40,), 10, start=1 << 20)
    ck = np.frombuffer(b"".join(chain), dtype=np.uint8).reshape(-1, ks)
    cv = rng.integers(0, 256, size=(10, vs), dtype=np.uint8)
    for k, v in zip(ck, cv):  # one by one: the chain's order is the insertion order
        vm.map_update_batch_device(m, dev(k[None, :].copy()), dev(v[None, :].copy()))
    ref_update(ref, m, ck, cv)
    check_lookup(vm, ref, m, ck, vs, dev, "colliding chain")
    found = vm.map_delete_batch(m, dev(ck[2:3].copy()))
    assert list(to_np(found)) == [1]
    ref_delete(ref, m, ck[2:3])
    check_lookup(vm, ref, m, ck, vs, dev, "chain with the third key deleted")  # (no host visit: the tombstone is live)
    nv = rng.integers(0, 256, size=(1, vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(ck[2:3].copy()), dev(nv))
    ref_update(ref, m, ck[2:3], nv)
    check_lookup(vm, ref, m, ck, vs, dev, "chain with the third key written again")
    check_lookup(vm, ref, m, np.ascontiguousarray(np.concatenate([keys, ck])), vs, dev, "both chains")
    same_map(vm, ref, m, "probe chains")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. duplicates
def run_duplicates(lib, oracle_lib, dev, ks: int = 13, vs: int = 24) -> None:
    rng = np.random.default_rng(3)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, HASH_MAX))
    pool = hash_pool(rng, ks, 4)
    keys = np.ascontiguousarray(np.repeat(pool[:1], 1000, axis=0))
    vals = np.ascontiguousarray((np.arange(1000 * vs, dtype=np.uint32) % 251).astype(np.uint8).reshape(1000, vs))
    vals[:, :4] = np.arange(1000, dtype=np.uint32).view(np.uint8).reshape(-1, 4)  # distinct values
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    ref_update(ref, m, keys, vals)
    same_map(vm, ref, m, "1,000 updates of one key")
    got, found = vm.map_lookup_batch(m, dev(pool[:1].copy()))
    assert list(to_np(found)) == [1] and np.array_equal(to_np(got)[0], vals[-1])
    vm.map_update_batch_device(m, dev(pool[1:3].copy()), dev(vals[:2].copy()))
    ref_update(ref, m, pool[1:3], vals[:2])
    before = vm.map_count(m)
    dk = np.ascontiguousarray(np.concatenate([np.repeat(pool[1:2], 7, axis=0), pool[3:4], pool[1:2]]))
    found = to_np(vm.map_delete_batch(m, dev(dk)))
    assert list(found) == [1] * 7 + [0, 1]
    ref_delete(ref, m, dk)
    assert vm.map_count(m) == before - 1
    same_map(vm, ref, m, "delete with a repeated key")
    vm.close()
    ref.close()


def run_tombstone_churn(lib, oracle_lib, dev, ks: int = 8, vs: int = 8) -> None:
    """Rounds of 64 fresh keys installed and deleted, with no host visit in between: the deleted records stay
    tombstones, so after two rounds the 128-slot table has no free record left. The next install still
    succeeds (the table is compacted through the host: one download, one upload) and nothing is lost."""
    rng = np.random.default_rng(11)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, HASH_MAX))
    pool = hash_pool(rng, ks, 5 * HASH_MAX)
    keep = np.ascontiguousarray(pool[:3])
    kv = rng.integers(0, 256, size=(3, vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(keep), dev(kv))
    ref_update(ref, m, keep, kv)
    up0, down0 = vm.map_traffic(m)
    for r in range(4):
        keys = np.ascontiguousarray(pool[HASH_MAX * (r + 1): HASH_MAX * (r + 1) + HASH_MAX - 3])
        vals = rng.integers(0, 256, size=(len(keys), vs), dtype=np.uint8)
        vm.map_update_batch_device(m, dev(keys), dev(vals))
        ref_update(ref, m, keys, vals)
        check_lookup(vm, ref, m, np.ascontiguousarray(np.concatenate([keys, keep])), vs, dev, f"churn round {r}")
        found = vm.map_delete_batch(m, dev(keys))
        assert to_np(found).all()
        ref_delete(ref, m, keys)
        check_lookup(vm, ref, m, np.ascontiguousarray(np.concatenate([keys, keep])), vs, dev, f"churn round {r}, deleted")
    up1, down1 = vm.map_traffic(m)
    assert down1 > down0 and up1 > up0, "the table ran out of free records without being compacted"
    same_map(vm, ref, m, "tombstone churn")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 4. limits
def rc_of(fn, *a) -> int:
    try:
        fn(*a)
    except EmulatorError as e:
        return e.rc
    return 0


def run_limits(lib, oracle_lib, dev, ks: int = 8, vs: int = 8) -> None:
    rng = np.random.default_rng(4)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, HASH_MAX))
    pool = hash_pool(rng, ks, HASH_MAX + 1)
    vals = rng.integers(0, 256, size=(HASH_MAX + 1, vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(pool[:HASH_MAX].copy()), dev(vals[:HASH_MAX].copy()))
    ref_update(ref, m, pool[:HASH_MAX], vals[:HASH_MAX])
    same_map(vm, ref, m, "filled to max_entries")
    before = vm.map_dump(m)
    k11 = np.ascontiguousarray(np.concatenate([pool[5:10], pool[HASH_MAX:], pool[20:25]]))  # 10 present keys, 1 new in between
    v11 = rng.integers(0, 256, size=(11, vs), dtype=np.uint8)
    assert rc_of(vm.map_update_batch_device, m, dev(k11), dev(v11)) == ERR_NOMEM
    after = vm.map_dump(m)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "a refused update changed the map"
    assert vm.map_count(m) == HASH_MAX
    check_lookup(vm, ref, m, np.ascontiguousarray(pool), vs, dev, "lookup after the refused update")
    k10, v10 = np.ascontiguousarray(np.delete(k11, 5, axis=0)), np.ascontiguousarray(np.delete(v11, 5, axis=0))
    vm.map_update_batch_device(m, dev(k10), dev(v10))
    ref_update(ref, m, k10, v10)
    same_map(vm, ref, m, "the same batch without the new key")
    # the refused batch left no claim behind: after a delete the new key fits
    vm.map_delete_batch(m, dev(pool[:1].copy()))
    ref_delete(ref, m, pool[:1])
    vm.map_update_batch_device(m, dev(k11), dev(v11))
    ref_update(ref, m, k11, v11)
    same_map(vm, ref, m, "the batch with the new key once it fits")
    vm.close()
    ref.close()

    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, ARRAY_MAX))
    idx = np.array([3, 99, ARRAY_MAX, 4], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    v4 = rng.integers(1, 256, size=(4, vs), dtype=np.uint8)
    assert rc_of(vm.map_update_batch_device, m, dev(idx), dev(v4)) == ERR_INVAL
    assert vm.map_dump(m) == bytes(ARRAY_MAX * vs), "a refused ARRAY update wrote something"
    assert rc_of(vm.map_delete_batch, m, dev(idx[:1].copy())) == ERR_INVAL  # as xe_map_delete
    assert not to_np(vm.map_lookup_batch(m, dev(idx))[0]).any()
    vm.close()
    ref.close()

    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        d = MapDef(t, 4, 8, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 8, 16)
        m = vm.add_map(d)
        k, v, f = np.zeros((2, 4), np.uint8), np.zeros((2, 8), np.uint8), np.zeros(2, np.uint8)
        assert lib.map_lookup_batch_device(vm.h, m, k.ctypes.data, 2, v.ctypes.data, f.ctypes.data, None) == ERR_UNSUPPORTED
        assert b"ARRAY and HASH" in lib.last_error(vm.h)
        assert lib.map_update_batch_device(vm.h, m, k.ctypes.data, v.ctypes.data, 2, None) == ERR_UNSUPPORTED
        assert lib.map_delete_batch_device(vm.h, m, k.ctypes.data, 2, f.ctypes.data, None) == ERR_UNSUPPORTED
        assert lib.map_lookup_batch(vm.h, m, k.ctypes.data, 2, v.ctypes.data, f.ctypes.data) == ERR_UNSUPPORTED
        assert lib.map_update_batch_staged(vm.h, m, k.ctypes.data, v.ctypes.data, 2) == ERR_UNSUPPORTED
        assert lib.map_delete_batch(vm.h, m, k.ctypes.data, 2, f.ctypes.data) == ERR_UNSUPPORTED
        vm.close()

    vm = VM(Settings(engine=1), lib=lib)
    m = vm.add_map(MapDef(MAP_HASH, 4, 8, 16))
    k, v = np.zeros((2, 4), np.uint8), np.zeros((2, 8), np.uint8)
    kp, vp = k.ctypes.data, v.ctypes.data
    assert lib.map_lookup_batch_device(vm.h, m, None, 2, vp, None, None) == ERR_INVAL
    assert lib.map_lookup_batch_device(vm.h, m, kp, 2, None, None, None) == ERR_INVAL
    assert lib.map_update_batch_device(vm.h, m, None, vp, 2, None) == ERR_INVAL
    assert lib.map_update_batch_device(vm.h, m, kp, None, 2, None) == ERR_INVAL
    assert lib.map_delete_batch_device(vm.h, m, None, 2, None, None) == ERR_INVAL
    assert lib.map_lookup_batch(vm.h, m, None, 2, vp, None) == ERR_INVAL
    assert lib.map_update_batch_staged(vm.h, m, kp, None, 2) == ERR_INVAL
    assert lib.map_delete_batch(vm.h, m, None, 2, None) == ERR_INVAL
    assert lib.map_lookup_batch_device(vm.h, 99, kp, 2, vp, None, None) == ERR_INVAL
    assert lib.map_lookup_batch_device(vm.h, m, None, 0, None, None, None) == 0  # count 0: nothing to do
    assert vm.map_count(m) == 0
    vm.close()


# ---------------------------------------------------------------- 5 - 7: a flow table under traffic
FLOW_PACKETS = 4099
FLOW_MAX = 16384


def flow_entries(fids) -> tuple[np.ndarray, np.ndarray]:
    fid = np.asarray(fids, dtype=np.uint64)
    keys = W.key_from_tuple(W.flow_tuples(3, fid))
    vals = np.zeros((len(fid), 16), dtype=np.uint8)
    vals[:, 0:8] = (fid + np.uint64(1)).view(np.uint8).reshape(-1, 8)
    return np.ascontiguousarray(keys), vals


def flow_vm(lib) -> tuple[VM, int]:
    """The C3-learn program (lookup, atomic add on a hit, bpf_map_update_elem on a miss) over an empty
    flow table."""
    vm = VM(Settings(engine=1), lib=lib)
    m = vm.add_map(MapDef(MAP_HASH, 16, 16, FLOW_MAX))
    vm.set_entrypoint(vm.add_raw_program(W.prog_c3learn()))
    return vm, m


class Runner:
    """Runs batches through the device-resident entry points, keeping the buffers alive."""

    def __init__(self, vm: VM, dev, use_async: bool):
        self.vm, self.dev, self.use_async, self.keep = vm, dev, use_async, []

    def run(self, start: int):
        umem, descs = W.build_batch("c3learn", start, FLOW_PACKETS)
        d_umem, d_desc = self.dev(umem), self.dev(descs.view(np.uint8).reshape(-1))
        d_ver = self.dev(np.zeros(FLOW_PACKETS, dtype=np.uint32))
        self.keep.append((d_umem, d_desc, d_ver))
        ptr = (lambda x: x.data_ptr()) if hasattr(d_umem, "data_ptr") else (lambda x: x.ctypes.data)
        run = self.vm.run_batch_device_async if self.use_async else self.vm.run_batch_device
        run(ptr(d_umem), len(umem), ptr(d_desc), FLOW_PACKETS, d_verdicts=ptr(d_ver))
        return d_ver  # (read after the next map call: those complete the pipeline)


def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    r = Runner(vm, dev, use_async)
    keys, vals = flow_entries(range(32))
    vm.map_update_batch_device(m, dev(keys), dev(vals))  # installs 32 flows
    ref_update(ref, rm, keys, vals)

    def ref_run(start: int) -> np.ndarray:
        umem, descs = W.build_batch("c3learn", start, FLOW_PACKETS)
        return ref.run_batch(umem, descs).verdicts

    v0 = r.run(0)
    w0 = ref_run(0)
    check_lookup(vm, ref, m, keys, 16, dev, "counters after the first batch")  # (no xe_sync before it)
    assert np.array_equal(to_np(v0), w0)
    assert to_np(vm.map_lookup_batch(m, dev(keys))[0])[:, 8:].any(), "no installed flow was hit"
    gone = np.ascontiguousarray(keys[4:12])
    found = vm.map_delete_batch(m, dev(gone))
    assert list(to_np(found)) == [1] * 8
    ref_delete(ref, rm, gone)
    v1 = r.run(FLOW_PACKETS)
    w1 = ref_run(FLOW_PACKETS)
    check_lookup(vm, ref, m, keys, 16, dev, "counters after the second batch")
    assert np.array_equal(to_np(v1), w1)
    same_map(vm, ref, m, "after two batches")  # the host dump ...
    for k in keys:  # ... and the single-key lookups
        assert vm.map_lookup(m, k.tobytes()) == ref.map_lookup(rm, k.tobytes())
    nk, nv = flow_entries([1 << 40])
    vm.map_update(m, nk[0].tobytes(), b"\x42" * 16)  # a host write, then a device read
    ref.map_update(rm, nk[0].tobytes(), b"\x42" * 16)
    check_lookup(vm, ref, m, np.ascontiguousarray(np.concatenate([nk, keys])), 16, dev, "device lookup after a host update")
    v2 = r.run(2 * FLOW_PACKETS)
    w2 = ref_run(2 * FLOW_PACKETS)
    same_map(vm, ref, m, "after three batches")
    assert np.array_equal(to_np(v2), w2)
    vm.close()
    ref.close()


def run_traffic(lib, dev) -> None:
    vm, m = flow_vm(lib)
    r = Runner(vm, dev, False)
    keys, vals = flow_entries(range(64))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    r.run(0)  # the map is now newer on the device
    up, down = vm.map_traffic(m)
    for _ in range(3):
        vm.map_lookup_batch(m, dev(keys))
    vm.map_update_batch_device(m, dev(keys[:16].copy()), dev(vals[:16].copy()))
    vm.map_delete_batch(m, dev(keys[16:24].copy()))
    assert vm.map_traffic(m) == (up, down), "a batched device call moved the whole map"
    r.run(FLOW_PACKETS)  # a batch after the device update: nothing to upload
    assert vm.map_traffic(m) == (up, down)
    assert vm.map_lookup(m, keys[0].tobytes()) is not None
    assert vm.map_traffic(m) == (up, down + 1), "the counter does not count the single-key path's download"
    vm.close()


def run_epoch(lib, dev) -> None:
    vm, m = flow_vm(lib)
    keys, vals = flow_entries(range(8))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    vm.epoch_begin()
    assert rc_of(vm.map_update_batch_device, m, dev(keys), dev(vals)) == ERR_INVAL
    assert rc_of(vm.map_delete_batch, m, dev(keys)) == ERR_INVAL
    got, found = vm.map_lookup_batch(m, dev(keys))
    assert list(to_np(found)) == [1] * 8 and np.array_equal(to_np(got), vals)
    vm.epoch_end()
    vm.map_delete_batch(m, dev(keys[:2].copy()))
    assert vm.map_count(m) == 6
    vm.close()
