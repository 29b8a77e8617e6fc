"""Shared cases of the batched device map operations (xe_map_lookup_batch_device / _update_ / _delete_):
tests/test_mapops.py runs them on the host simulation, tests/test_mapops_gpu.py on the product library.

Every expected value comes from an oracle VM (oracle/liboracle.so) given the same operations through its
single-key map_update / map_lookup / map_delete, in batch order; map_dump (sorted by key) and map_count
are compared after every step. VMs run the shared interpreter (engine=1): nothing compiles.

`dev` turns a numpy array into what the VM methods take for device memory: the array itself on the host
simulation (device addresses are host addresses there), a CUDA tensor on the product.

Sections 1 to 7 are the everyday shapes. Sections 8 to 11 go where the kernels branch and the everyday
shapes do not: the value and key sizes on both sides of every cut (EDGE_PAIRS), the empty key, buffers that
are not 16-byte aligned (with guard bytes around them), tens of thousands of distinct keys claimed,
deleted, claimed again and refused in single launches, and nil-backed HASH values. The host simulation
runs one entry after another, so the lane sub-groups, the vector moves and the races of those sections
exist on the device only; the simulation still pins down what the right answer is."""
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
# The sizes at which the kernels take another path (xe_mapops.h xe_mo_lanes: 1, 4, 16 or 64 lanes per value,
# cut at 16, 64 and 1024 bytes; xe_mapops.hip find_slot: the empty key, 2-word records up to 8 key bytes,
# 4-word records up to 24, 8-word records up to 56), one on each side of every cut.
EDGE_VALUE_SIZES = (16, 17, 64, 65, 1024, 1025)
EDGE_KEY_SIZES = (0, 16, 17, 24, 25, 56)
EDGE_PAIRS = tuple(dict.fromkeys([(ks, vs) for vs in EDGE_VALUE_SIZES for ks in (8, 24)] +
                                 [(ks, vs) for ks in EDGE_KEY_SIZES for vs in (8, 65)]))
# 257: the smallest count that needs a second workgroup at one entry per lane (17 workgroups of the 16-lane
# value kernel); 4099: prime, many workgroups of every sub-group width
EDGE_COUNTS = (0, 1, 63, 64, 65, 257, 4099)
GUARD_KEY_SIZES = KEY_SIZES + (16, 17, 24, 25, 56)
SLOT_FULL, SLOT_VLEN0, SLOT_TOMB, SLOT_BUSY = 1, 2, 4, 8  # xe_internal.h XE_SLOT_*


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
def run_matrix(lib, oracle_lib, dev, kind: int, ks: int, vs: int, counts=COUNTS) -> None:
    if kind == MAP_HASH and ks == 0:
        return run_empty_key(lib, oracle_lib, dev, vs)
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
    for n in counts:
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
        if n == counts[-1]:
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


# ---------------------------------------------------------------- device memory by address
def on_dev(x) -> bool:
    return hasattr(x, "data_ptr")


def addr(x) -> int:
    return x.data_ptr() if on_dev(x) else x.ctypes.data


def settle(x) -> None:
    """The library works on a stream of its own: whatever torch queued to fill x completes first."""
    if on_dev(x):
        import torch
        torch.cuda.synchronize()


GUARD = 0xEE


def place(dev, arr: np.ndarray, off: int, tail: int = 48):
    """(buffer, view): arr's bytes at byte offset `off` of a buffer that starts on a 16-byte boundary and
    is GUARD everywhere else. The view (a numpy view / a tensor slice) is what a call is given."""
    flat = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    size = off + flat.size + tail
    raw = np.full(size + 16, GUARD, dtype=np.uint8)
    shift = (-raw.ctypes.data) % 16
    host = raw[shift:shift + size]
    host[off:off + flat.size] = flat
    buf = dev(host)
    assert addr(buf) % 16 == 0 and len(buf) == size
    return buf, buf[off:off + flat.size]


def guards_intact(buf, off: int, nbytes: int, what: str) -> np.ndarray:
    """The buffer on the host, after checking that every byte outside [off, off + nbytes) is still GUARD."""
    got = to_np(buf)
    assert (got[:off] == GUARD).all(), f"{what}: bytes in front of the buffer were written"
    assert (got[off + nbytes:] == GUARD).all(), f"{what}: bytes behind the buffer were written"
    return got[off:off + nbytes]


def unchanged(buf, off: int, arr: np.ndarray, what: str) -> None:
    got = guards_intact(buf, off, arr.size, what)
    assert np.array_equal(got, np.ascontiguousarray(arr).view(np.uint8).reshape(-1)), f"{what}: an input buffer changed"


# ---------------------------------------------------------------- the map's records, without a host visit
def hash_geometry(vm: VM, m: int):
    """(cap, record words, bytes of the value region) of a HASH map's state image
    ([values][cap + 1 records][count u32, pad], xe_map_state_export)."""
    d = vm.map_defs[m]
    rw, nbytes = rwords(d.key_size), vm.map_state_bytes(m)
    cap = 16
    while True:
        vals_alloc = max(8, ((cap + 1) * d.value_size + 7) & ~7)
        if vals_alloc + (cap + 1) * rw * 8 + 8 >= nbytes:
            break
        cap <<= 1
    assert vals_alloc + (cap + 1) * rw * 8 + 8 == nbytes and cap >= d.max_entries
    return cap, rw, vals_alloc


def state_image(vm: VM, m: int, dev) -> np.ndarray:
    """xe_map_state_export into memory of the library's kind, then on the host. Device-to-device: the map
    does not visit the host, so tombstones and reservations stay where they are."""
    buf = dev(np.zeros(vm.map_state_bytes(m), dtype=np.uint8))
    settle(buf)
    vm.map_state_export(m, addr(buf))
    return to_np(buf).copy()


def image_records(vm: VM, m: int, img: np.ndarray):
    """(word 0 of every record, key bytes of every record, value bytes of every record, count) of a HASH image.
    Between calls no record is BUSY and every last-writer word (the high half of word 0) is zero."""
    d = vm.map_defs[m]
    cap, rw, vals_alloc = hash_geometry(vm, m)
    rec = img[vals_alloc:vals_alloc + (cap + 1) * rw * 8].view(np.uint64).reshape(cap + 1, rw)
    w0 = rec[:, 0]
    assert not (w0 >> np.uint64(32)).any(), "a last-writer word was left behind"
    assert not (w0 & np.uint64(SLOT_BUSY)).any(), "a claim was left behind"
    keys = np.ascontiguousarray(rec[:, 1:]).view(np.uint8).reshape(cap + 1, (rw - 1) * 8)[:, :d.key_size]
    vals = img[:(cap + 1) * d.value_size].reshape(cap + 1, d.value_size)
    return w0, keys, vals, int(img[-8:-4].view(np.uint32)[0])


def by_key(keys: np.ndarray, vals: np.ndarray):
    order = np.lexsort(keys.T[::-1]) if keys.shape[1] else np.arange(len(keys))
    return keys[order], vals[order]


def same_image_map(vm: VM, ref: VM, m: int, dev, what: str) -> np.ndarray:
    """The FULL records of the exported image against the oracle's dump and count: same_map without the
    host visit that map_dump makes (which rebuilds the table without its tombstones). Returns the image."""
    img = state_image(vm, m, dev)
    w0, keys, vals, count = image_records(vm, m, img)
    full = np.nonzero(w0 & np.uint64(SLOT_FULL))[0]
    gv = vals[full].copy()
    gv[(w0[full] & np.uint64(SLOT_VLEN0)) != 0] = 0
    gk, gv = by_key(keys[full], gv)
    wk, wv = by_key(*ref.map_dump(m))
    assert count == len(full) == ref.map_count(m), f"{what}: count differs ({count}, {len(full)}, {ref.map_count(m)})"
    assert np.array_equal(gk, wk), f"{what}: keys differ"
    assert np.array_equal(gv, wv), f"{what}: values differ"
    return img


# ---------------------------------------------------------------- 8. the empty key
def run_empty_key(lib, oracle_lib, dev, vs: int) -> None:
    """A HASH map with key_size 0 holds one entry, in the record past the table (xe_mapops.h mo_find,
    mo_update_locate_item `single`; xe_mapops.hip find_slot). hash_pool cannot make distinct empty keys:
    batches of 1, 3 and 300 empty keys with distinct values, the last of which wins. The calls are made by
    address (an empty key array has none of its own: any readable address serves)."""
    rng = np.random.default_rng(8000 + vs)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 0, vs, HASH_MAX))
    some = dev(np.zeros(64, dtype=np.uint8))
    device = on_dev(some)

    def update(vals):
        d_v = dev(vals)
        settle(d_v)
        if device:
            return lib.map_update_batch_device(vm.h, m, addr(some), addr(d_v), len(vals), None)
        return lib.map_update_batch_staged(vm.h, m, addr(some), addr(d_v), len(vals))

    def lookup(n):
        d_v, d_f = dev(np.full((n, vs), GUARD, np.uint8)), dev(np.full(n, GUARD, np.uint8))
        settle(d_v)
        if device:
            rc = lib.map_lookup_batch_device(vm.h, m, addr(some), n, addr(d_v), addr(d_f), None)
        else:
            rc = lib.map_lookup_batch(vm.h, m, addr(some), n, addr(d_v), addr(d_f))
        assert rc == 0, lib.last_error(vm.h)
        return to_np(d_v), to_np(d_f)

    def delete(n):
        d_f = dev(np.full(n, GUARD, np.uint8))
        settle(d_f)
        if device:
            rc = lib.map_delete_batch_device(vm.h, m, addr(some), n, addr(d_f), None)
        else:
            rc = lib.map_delete_batch(vm.h, m, addr(some), n, addr(d_f))
        assert rc == 0, lib.last_error(vm.h)
        return to_np(d_f)

    got, found = lookup(2)
    assert ref.map_lookup(m, b"") is None and list(found) == [0, 0] and not got.any()
    for n in (1, 3, 300):
        vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
        vals[:, 0] = np.arange(n) % 251 + 1  # distinct, none zero
        assert update(vals) == 0, lib.last_error(vm.h)
        for v in vals:
            ref.map_update(m, b"", v.tobytes())
        want = ref.map_lookup(m, b"")
        assert want == vals[-1].tobytes()
        got, found = lookup(5)
        assert list(found) == [1] * 5 and all(g.tobytes() == want for g in got), f"empty key after a batch of {n}"
        assert vm.map_count(m) == ref.map_count(m) == 1
        same_map(vm, ref, m, f"empty key after a batch of {n}")
        assert vm.map_lookup(m, b"") == want
    assert list(delete(3)) == [1, 1, 1]
    ref.map_delete(m, b"")
    assert vm.map_count(m) == ref.map_count(m) == 0
    got, found = lookup(3)
    assert list(found) == [0, 0, 0] and not got.any() and ref.map_lookup(m, b"") is None
    assert list(delete(2)) == [0, 0]
    same_map(vm, ref, m, "empty key deleted")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 9. alignment, with guard bytes
# Fresh allocations are at least 16-byte aligned, so mo_load_key's word path and mo_move's choice of unit
# (16, 8 or 4 bytes or single bytes, by how source and destination are aligned to each other, with a head
# up to the first aligned byte and a tail) never vary with them. Here keys, values and outputs sit 0, 1, 4
# or 8 bytes past a 16-byte boundary inside buffers of GUARD bytes. Value sizes 24 and 64 keep map storage
# 8-byte aligned (16- and 8-byte units, a head of 8); 100 puts every other value 4 bytes off (8-byte units
# with a head of 4); 4097 runs through every relative alignment (4-byte units with heads of 1 to 3).
ALIGN_OFFSETS = ((0, 0), (1, 1), (4, 4), (8, 8), (8, 1), (1, 8))  # (keys and found, values)
ALIGN_HASH = ((8, 8), (8, 24), (16, 64), (24, 100), (8, 4097))
ALIGN_ARRAY = (24, 64, 100)
ALIGN_N = 257


def run_alignment(lib, oracle_lib, dev, kind: int, ks: int, vs: int) -> None:
    array = kind == MAP_ARRAY
    for koff, voff in ALIGN_OFFSETS:
        what = f"keys at +{koff}, values at +{voff}"
        rng = np.random.default_rng(100000 + 1000 * ks + vs + 16 * koff + voff)
        n = ALIGN_N
        vm, ref, m, _ = pair(lib, oracle_lib, MapDef(kind, 4 if array else ks, vs, ARRAY_MAX if array else 2 * n))
        if array:
            keys = rng.integers(0, ARRAY_MAX, size=n, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
            absent = np.array([ARRAY_MAX, ARRAY_MAX + 1, 0xffffffff], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
        else:
            both = hash_pool(rng, ks, n + 16)
            keys, absent = both[:n], both[n:]
        vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
        kbuf, kview = place(dev, keys, koff)
        vbuf, vview = place(dev, vals, voff)
        settle(vbuf)
        # (by address: the calls that take arrays stage host memory through aligned buffers of the VM's)
        rc = lib.map_update_batch_device(vm.h, m, addr(kview), addr(vview), n, None)
        assert rc == 0, lib.last_error(vm.h)
        ref_update(ref, m, keys, vals)
        unchanged(kbuf, koff, keys, f"update, {what}: keys")
        unchanged(vbuf, voff, vals, f"update, {what}: values")

        probe = np.ascontiguousarray(np.concatenate([keys[rng.permutation(n)], absent]))
        pbuf, pview = place(dev, probe, koff)
        obuf, oview = place(dev, np.full((len(probe), vs), GUARD, np.uint8), voff)
        fbuf, fview = place(dev, np.full(len(probe), GUARD, np.uint8), koff)
        settle(obuf)
        rc = lib.map_lookup_batch_device(vm.h, m, addr(pview), len(probe), addr(oview), addr(fview), None)
        assert rc == 0, lib.last_error(vm.h)
        wv, wf = ref_lookup(ref, m, probe, vs)
        got = guards_intact(obuf, voff, wv.size, f"lookup, {what}: values")
        assert np.array_equal(guards_intact(fbuf, koff, len(probe), f"lookup, {what}: found"), wf), f"lookup, {what}: found differs"
        assert np.array_equal(got.reshape(-1, vs), wv), f"lookup, {what}: values differ"
        unchanged(pbuf, koff, probe, f"lookup, {what}: keys")
        same_map(vm, ref, m, f"update, {what}")
        if not array:
            dk = np.ascontiguousarray(np.concatenate([keys[::3], absent[:3], keys[:2]]))
            _, present = ref_lookup(ref, m, dk, vs)
            dbuf, dview = place(dev, dk, koff)
            gbuf, gview = place(dev, np.full(len(dk), GUARD, np.uint8), voff)
            settle(gbuf)
            rc = lib.map_delete_batch_device(vm.h, m, addr(dview), len(dk), addr(gview), None)
            assert rc == 0, lib.last_error(vm.h)
            assert np.array_equal(guards_intact(gbuf, voff, len(dk), f"delete, {what}: found"), present), f"delete, {what}: found differs"
            unchanged(dbuf, koff, dk, f"delete, {what}: keys")
            ref_delete(ref, m, dk)
            check_lookup(vm, ref, m, probe, vs, dev, f"lookup after the delete, {what}")
            same_map(vm, ref, m, f"delete, {what}")
        vm.close()
        ref.close()


# ---------------------------------------------------------------- 10. contention at scale
# What the host loop cannot show: thousands of waves of one launch claiming records for different keys
# (mo_update_locate_item: the CAS that is lost and tried again, the BUSY record that names another entry),
# the per-wave count of the claims, the delete's claim raced by repetitions, and the UNDO of all of it.
# Every step is compared with the oracle replaying the same entries in batch order: the FULL records of the
# exported state image (same_image_map: no host visit, so the tombstones of step b are still there when c
# and d claim them), and a lookup of every key touched so far plus 1,000 absent ones. map_dump and
# map_count, which visit the host, are compared where no later step needs the tombstones.
CONT_KS, CONT_VS, CONT_MAX = 16, 40, 32768


def distinct_values(rng, n: int, vs: int) -> np.ndarray:
    v = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    v[:, :4] = np.arange(1, n + 1, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    return v


def run_contention(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(10)
    ks, vs = CONT_KS, CONT_VS
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, CONT_MAX))
    pool = hash_pool(rng, ks, 42000)
    first, absent, del_absent, fresh_c, fresh_d = pool[:30000], pool[30000:31000], pool[31000:32000], pool[32000:37000], pool[37000:42000]
    touched = [absent]

    def step(keys, what, host_visit=False):
        touched.append(keys)
        img = same_image_map(vm, ref, m, dev, what)
        allk = np.unique(np.concatenate(touched), axis=0)
        check_lookup(vm, ref, m, np.ascontiguousarray(allk), vs, dev, what)
        if host_visit:
            same_map(vm, ref, m, what)
        return img

    def shuffled(*parts):
        k = np.concatenate(parts)
        return np.ascontiguousarray(k[rng.permutation(len(k))])

    # a: 50,000 entries in flight at once (below the 65,536 of one pass of the grid): 30,000 distinct keys, the
    # first 10,000 three times each
    ka = shuffled(first, first[:10000], first[:10000])
    va = distinct_values(rng, len(ka), vs)
    assert len(ka) == 50000
    vm.map_update_batch_device(m, dev(ka), dev(va))
    ref_update(ref, m, ka, va)
    assert ref.map_count(m) == 30000
    step(ka, "a: 50,000 updates of 30,000 keys", host_visit=True)  # (no tombstone yet: the visit changes nothing)

    # b: 15,000 present keys, 5,000 of them twice, and 1,000 absent ones
    gone = first[5000:20000]
    kb = shuffled(gone, gone[:5000], del_absent)
    _, present = ref_lookup(ref, m, kb, vs)
    assert present.sum() == 20000
    found = to_np(vm.map_delete_batch(m, dev(kb)))
    assert np.array_equal(found, present), "b: found differs (1 for every repetition of a present key)"
    ref_delete(ref, m, kb)
    assert ref.map_count(m) == 15000
    img = step(kb, "b: 21,000 deletes")
    assert int((image_records(vm, m, img)[0] & np.uint64(SLOT_TOMB) != 0).sum()) == 15000

    # c: 10,000 of the deleted keys (their records are reservations now), 3,000 of them twice, and 5,000 fresh keys
    back = gone[:10000]
    kc = shuffled(back, back[2000:5000], fresh_c)
    vc = distinct_values(rng, len(kc), vs)
    vm.map_update_batch_device(m, dev(kc), dev(vc))
    ref_update(ref, m, kc, vc)
    assert ref.map_count(m) == 30000
    img = step(kc, "c: 18,000 updates over reservations")
    # the 10,000 took their own records again: the 5,000 deleted keys that did not come back are the tombstones left
    assert int((image_records(vm, m, img)[0] & np.uint64(SLOT_TOMB) != 0).sum()) == 5000

    # d: does not fit. 3,000 present keys, 2,000 tombstone claims, 5,000 fresh keys (room for 2,768), 500
    # repetitions of each kind
    room = CONT_MAX - 30000
    here, tomb = first[:3000], gone[10000:12000]
    assert len(fresh_d) >= room + 1000
    kd = shuffled(here, tomb, fresh_d, here[:500], tomb[:500], fresh_d[:500])
    vd = distinct_values(rng, len(kd), vs)
    before = state_image(vm, m, dev)
    assert rc_of(vm.map_update_batch_device, m, dev(kd), dev(vd)) == ERR_NOMEM
    after = state_image(vm, m, dev)
    assert np.array_equal(before, after), "d: a refused update left the state image changed"
    assert image_records(vm, m, after)[3] == 30000
    step(kd, "d: the refused batch", host_visit=True)
    assert vm.map_count(m) == ref.map_count(m) == 30000

    # e: the same batch with only as many new keys as there is room for
    keep = np.ones(len(kd), dtype=bool)
    drop = {k.tobytes() for k in fresh_d[room - len(tomb):]}
    for i, k in enumerate(kd):
        keep[i] = k.tobytes() not in drop
    ke, ve = np.ascontiguousarray(kd[keep]), np.ascontiguousarray(vd[keep])
    vm.map_update_batch_device(m, dev(ke), dev(ve))
    ref_update(ref, m, ke, ve)
    step(ke, "e: the batch cut down to fit", host_visit=True)
    assert vm.map_count(m) == ref.map_count(m) == CONT_MAX
    vm.close()
    ref.close()

    # the refused ARRAY update at the same scale: 4,099 entries, one index out of range in the middle
    n, amax = 4099, 1000
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, amax))
    idx = rng.integers(0, amax, size=n, dtype=np.uint32)
    v0 = distinct_values(rng, n, vs)
    vm.map_update_batch_device(m, dev(idx.view(np.uint8).reshape(-1, 4)), dev(v0))
    ref_update(ref, m, idx.view(np.uint8).reshape(-1, 4), v0)
    same_map(vm, ref, m, "ARRAY update of 4,099")
    bad = rng.integers(0, amax, size=n, dtype=np.uint32)
    bad[n // 2] = amax
    assert rc_of(vm.map_update_batch_device, m, dev(bad.view(np.uint8).reshape(-1, 4)), dev(distinct_values(rng, n, vs))) == ERR_INVAL
    same_map(vm, ref, m, "ARRAY update refused for one index of 4,099")
    bad[n // 2] = 0  # ... and the same batch without it goes through: nothing of the refused one is in the way
    v1 = distinct_values(rng, n, vs)
    vm.map_update_batch_device(m, dev(bad.view(np.uint8).reshape(-1, 4)), dev(v1))
    ref_update(ref, m, bad.view(np.uint8).reshape(-1, 4), v1)
    same_map(vm, ref, m, "ARRAY update after the refused one")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 11. nil-backed HASH values
def run_vlen0(lib, oracle_lib, dev) -> None:
    """A HASH value written from an unreadable range has a nil backing: the record carries XE_SLOT_VLEN0
    and reads as zeros, while its stored bytes are still the earlier value. The program and packets of
    test_lru_nil_value.py over a HASH map leave three of the four keys like that; the batched lookup reads
    them (kMoVlen0), and a batched update publishes over two of them (COPY clears the flag)."""
    from parity import packets
    from test_lru_nil_value import _program
    umem, descs = packets(600, 64, seed=9)
    for d in descs:
        umem[int(d["addr"]) + 1] = 0
    nil = set()
    for i in (150, 151, 400):
        umem[int(descs[i]["addr"]) + 1] = 1
        nil.add(int(umem[int(descs[i]["addr"])]) & 3)
    nil = sorted(nil)
    assert len(nil) == 3
    vms = []
    for lb in (lib, oracle_lib):
        vm = VM(Settings(engine=1), lib=lb)
        m = vm.add_map(MapDef(MAP_HASH, 4, 8, 16))
        vm.set_entrypoint(vm.add_raw_program(_program()))
        vms.append((vm, vm.run_batch(umem.copy(), descs)))
    (vm, got), (ref, want) = vms
    assert np.array_equal(got.verdicts, want.verdicts)
    w0 = image_records(vm, m, state_image(vm, m, dev))[0]
    assert int((w0 & np.uint64(SLOT_VLEN0) != 0).sum()) == 3, "the batch left no nil-backed records on the device"
    keys = np.array([0, 1, 2, 3, 77], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vals, found = vm.map_lookup_batch(m, dev(keys))
    assert list(to_np(found)) == [1, 1, 1, 1, 0]
    assert not to_np(vals)[nil].any() and to_np(vals)[[k for k in range(4) if k not in nil]].any()
    check_lookup(vm, ref, m, keys, 8, dev, "lookup of nil-backed values")
    k2 = np.ascontiguousarray(keys[nil[:2]])
    v2 = np.array([[0x11] * 8, [0x22] * 8], dtype=np.uint8)
    vm.map_update_batch_device(m, dev(k2), dev(v2))
    ref_update(ref, m, k2, v2)
    check_lookup(vm, ref, m, keys, 8, dev, "lookup after an update over nil-backed values")
    same_map(vm, ref, m, "update over nil-backed values")
    for k in keys:
        assert vm.map_lookup(m, k.tobytes()) == ref.map_lookup(m, k.tobytes())
    vm.close()
    ref.close()
