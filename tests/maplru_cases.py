"""Shared cases of the device-side LRU_HASH calls (xe_lru_lookup_batch_device, xe_lru_delete_batch_device,
xe_lru_order_device, xe_lru_evict_device and the host-pointer forms): tests/test_maplru.py runs them on the host
simulation, tests/test_maplru_gpu.py on the product library.

No expected value comes from the code under test. A second VM on the oracle library holds the same initial map
and gets the same keys one at a time (xe_map_lookup promotes, xe_map_delete removes); what order and evict must
report is computed in numpy from the oracle's xe_map_lru_order and xe_map_dump (the eligible entries by
mapscan_cases.selects, the first r of the usage order or of its reverse). found, values, the usage order, the
dump and the count are compared for equality.

`dev` is mapscan_cases': a numpy array stays one on the host simulation and becomes a CUDA tensor on the
product; host_form sends a call through the host-pointer forms. Batches run on the interpreter engine, so no
test compiles a per-program kernel.

Sizes (xe_mapops.h): a tile is 256 slots in 4 rounds of 64 (LIVE_EDGES), a lane step takes one key per lane
and a wave is 64 of them (COUNTS), and the value sizes are one per xe_mo_lanes class."""
from __future__ import annotations

import ctypes as C

import numpy as np

from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (ENGINE_INTERP, MAP_HASH, MAP_LRU_HASH, MODE_SEQUENTIAL, VM, EmulatorError, MapDef, MapFilter,
                                  Settings)
from mapops_cases import GUARD, addr, guards_intact, hash_pool, place, rc_of, settle, to_np
from mapscan_cases import ALL, EQ, NE, OPS, selects

ERR_INVAL, ERR_UNSUPPORTED = -22, -95  # include/xdpemu.h XE_ERR_*
PEEK, OLDEST = 1, 1
# (key_size, value_size, max_entries): every key size, value size (one per xe_mo_lanes class) and table size once
GEOMETRY = ((4, 8, 16), (13, 24, 300), (64, 100, 4096), (4, 1100, 300), (13, 8, 4096))
COUNTS = (0, 1, 63, 64, 65, 257)
LIVE_EDGES = (0, 1, 255, 256, 257)
STATES = ("parallel_batch", "one_lane_replay", "fresh_upload", "epoch_wrap")


# ---------------------------------------------------------------- the two VMs
def lru_pair(lib, oracle_lib, ks: int, vs: int, max_entries: int, settings=None):
    d = MapDef(MAP_LRU_HASH, ks, vs, max_entries)
    vm, ref = VM(settings or Settings(engine=ENGINE_INTERP), lib=lib), VM(Settings(), lib=oracle_lib)
    return vm, ref, vm.add_map(d), ref.add_map(d)


def fill(vm: VM, ref: VM, m: int, keys: np.ndarray, vals: np.ndarray) -> None:
    """The same entries into both maps through the host calls (the last key is the most recently used)."""
    if len(keys):
        vm.map_update_batch(m, keys, vals)
        ref.map_update_batch(m, keys, vals)


def entries(rng, ks: int, vs: int, n: int):
    keys = hash_pool(rng, ks, n + 8)  # (the last 8 never enter the map: absent keys)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    return keys[:n], vals, keys[n:]


def same_lru(vm: VM, ref: VM, m: int, what: str) -> None:
    got, want = vm.map_lru_order(m), ref.map_lru_order(m)
    assert got == want, f"{what}: the usage order differs"
    (gk, gv), (wk, wv) = vm.map_dump(m), ref.map_dump(m)
    assert np.array_equal(gk, wk), f"{what}: keys differ"
    assert np.array_equal(gv, wv), f"{what}: values differ"
    assert vm.map_count(m) == ref.map_count(m), f"{what}: count differs"


def ref_lookup(ref: VM, m: int, keys: np.ndarray, vs: int):
    """(values, found) of the oracle's single-key lookups in batch order: each one promotes."""
    vals = np.zeros((len(keys), vs), dtype=np.uint8)
    found = np.zeros(len(keys), dtype=np.uint8)
    for i, k in enumerate(keys):
        v = ref.map_lookup(m, k.tobytes())
        if v is not None:
            vals[i] = np.frombuffer(v, dtype=np.uint8)
            found[i] = 1
    return vals, found


def ref_peek(ref: VM, m: int, keys: np.ndarray, vs: int):
    """(values, found) from the oracle's dump: no state changes."""
    dk, dv = ref.map_dump(m)
    table = {k.tobytes(): v for k, v in zip(dk, dv)}
    vals = np.zeros((len(keys), vs), dtype=np.uint8)
    found = np.zeros(len(keys), dtype=np.uint8)
    for i, k in enumerate(keys):
        if k.tobytes() in table:
            vals[i] = table[k.tobytes()]
            found[i] = 1
    return vals, found


def check_lookup(vm: VM, ref: VM, m: int, keys: np.ndarray, dev, what: str, peek: bool = False) -> None:
    vs = vm.map_defs[m].value_size
    keys = np.array(keys, dtype=np.uint8, order="C", copy=True)  # (a reversed view of one row passes for contiguous)
    vals, found = vm.lru_lookup_batch(m, dev(keys), peek=peek)
    wv, wf = (ref_peek if peek else ref_lookup)(ref, m, keys, vs)
    assert np.array_equal(to_np(found), wf), f"{what}: found differs"
    assert np.array_equal(to_np(vals), wv), f"{what}: values differ"
    same_lru(vm, ref, m, what)


def check_delete(vm: VM, ref: VM, m: int, keys: np.ndarray, dev, what: str) -> None:
    keys = np.array(keys, dtype=np.uint8, order="C", copy=True)
    _, wf = ref_peek(ref, m, keys, vm.map_defs[m].value_size)  # present before the call, for every repetition
    found = vm.lru_delete_batch(m, dev(keys))
    for k in keys:
        ref.map_delete(m, k.tobytes())
    assert np.array_equal(to_np(found), wf), f"{what}: found differs"
    same_lru(vm, ref, m, what)


# ---------------------------------------------------------------- order / evict: the answer, and the calls
def expect_order(ref: VM, m: int, flt, oldest: bool, k: int):
    """(keys[r], values[r], matched) from the oracle's usage order and dump."""
    d = ref.map_defs[m]
    order = ref.map_lru_order(m)
    dk, dv = ref.map_dump(m)
    table = {kk.tobytes(): v for kk, v in zip(dk, dv)}
    keys = np.frombuffer(b"".join(order), dtype=np.uint8).reshape(-1, d.key_size) if order else np.zeros((0, d.key_size), np.uint8)
    vals = np.array([table[kb] for kb in order], dtype=np.uint8).reshape(-1, d.value_size)
    if oldest:
        keys, vals = keys[::-1], vals[::-1]
    pick = np.nonzero(selects(vals, flt))[0]
    r = min(k, len(pick))
    return np.ascontiguousarray(keys[pick[:r]]), np.ascontiguousarray(vals[pick[:r]]), len(pick)


def c_filter(flt):
    return None if flt is None else (flt if isinstance(flt, N.MapFilter) else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand))


def raw_order(lib, vm: VM, m: int, flt, flags: int, kptr, vptr, k: int, device_form: bool = True, evict: bool = False, matched: bool = True):
    """One call by address. Returns (rc, matched)."""
    cf = c_filter(flt)
    n = C.c_uint64(0xDEADBEEF)
    head = (vm.h, m, None if cf is None else C.byref(cf), flags, kptr or None, vptr or None, k, C.byref(n) if matched else None)
    if device_form:
        return (lib.lru_evict_device if evict else lib.lru_order_device)(*head, None), n.value
    return (lib.lru_evict if evict else lib.lru_order)(*head), n.value


def call_order(lib, vm: VM, m: int, dev, flt, oldest: bool, k: int, room: int, evict: bool = False, koff: int = 0, voff: int = 0,
               want_keys: bool = True, want_vals: bool = True, host_form: bool = False):
    """An order or an evict into GUARD buffers of `room` entries, koff / voff bytes past a 16-byte boundary.
    Returns (keys[r], values[r], matched) after checking that no byte in front of the buffers or behind entry r
    was written."""
    d = vm.map_defs[m]
    ks, vs = d.key_size, d.value_size
    mk = np.ascontiguousarray if host_form else dev
    kbuf, _ = place(mk, np.full((room, ks), GUARD, np.uint8), koff)
    vbuf, _ = place(mk, np.full((room, vs), GUARD, np.uint8), voff)
    settle(kbuf)
    settle(vbuf)
    rc, matched = raw_order(lib, vm, m, flt, OLDEST if oldest else 0, addr(kbuf) + koff if want_keys else 0,
                            addr(vbuf) + voff if want_vals else 0, k, not host_form, evict)
    assert rc == 0, lib.last_error(vm.h)
    r = min(matched, k)
    assert r <= room
    what = f"{'evict' if evict else 'order'} k {k}, keys +{koff}, values +{voff}"
    kk = guards_intact(kbuf, koff, r * ks if want_keys else 0, what + ": keys").reshape(-1, ks)
    v = guards_intact(vbuf, voff, r * vs if want_vals else 0, what + ": values").reshape(-1, vs)
    return kk, v, matched


def check_order(lib, vm: VM, ref: VM, m: int, dev, k: int, flt=None, oldest: bool = False, evict: bool = False, **kw) -> int:
    """One order or evict against the oracle; an evict's keys are then deleted there one by one and the maps
    compared. Returns r."""
    ek, ev, matched = expect_order(ref, m, flt, oldest, k)
    gk, gv, gm = call_order(lib, vm, m, dev, flt, oldest, k, len(ek) + 3, evict, **kw)
    what = f"{'evict' if evict else 'order'} k {k} oldest {oldest} filter {flt}"
    assert gm == matched, f"{what}: matched {gm}, expected {matched}"
    if kw.get("want_keys", True):
        assert np.array_equal(gk, ek), f"{what}: keys differ (or their order)"
    if kw.get("want_vals", True):
        assert np.array_equal(gv, ev), f"{what}: values differ (or their order)"
    if evict:
        for kk in ek:
            ref.map_delete(m, kk.tobytes())
        same_lru(vm, ref, m, what)
    return len(ek)


# ---------------------------------------------------------------- 1. geometry
def run_geometry(lib, oracle_lib, dev, ks: int, vs: int, max_entries: int) -> None:
    """Every count against one map: lookups (present, absent and repeated keys mixed), peeks, deletes, and both
    orders; the map fills to max_entries first."""
    rng = np.random.default_rng(ks * 7919 + vs)
    vm, ref, m, _ = lru_pair(lib, oracle_lib, ks, vs, max_entries)
    keys, vals, absent = entries(rng, ks, vs, max_entries)
    fill(vm, ref, m, keys, vals)
    for n in COUNTS:
        pick = rng.integers(0, len(keys), size=n)
        batch = keys[pick].copy()
        if n:
            batch[rng.integers(0, n, size=max(1, n // 8))] = absent[rng.integers(0, len(absent), size=max(1, n // 8))]
        check_lookup(vm, ref, m, batch, dev, f"lookup of {n} keys")
        check_lookup(vm, ref, m, batch[::-1], dev, f"peek of {n} keys", peek=True)
    for oldest in (False, True):
        check_order(lib, vm, ref, m, dev, max_entries + 1, oldest=oldest)
        check_order(lib, vm, ref, m, dev, 5, oldest=oldest, host_form=True)
    for n in COUNTS:
        live = [np.frombuffer(k, np.uint8) for k in ref.map_lru_order(m)]
        if not live:
            break
        batch = np.array([live[i] for i in rng.integers(0, len(live), size=n)], dtype=np.uint8).reshape(n, ks)
        if n:
            batch[0] = absent[0]
        check_delete(vm, ref, m, batch, dev, f"delete of {n} keys")
    check_order(lib, vm, ref, m, dev, max_entries, oldest=True)
    check_lookup(vm, ref, m, keys[: min(70, len(keys))], dev, "lookup after the deletes")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. live entries at the tile edges
def run_live_edge(lib, oracle_lib, dev, live: int) -> None:
    rng = np.random.default_rng(live)
    vm, ref, m, _ = lru_pair(lib, oracle_lib, 8, 24, 300)
    keys, vals, absent = entries(rng, 8, 24, live)
    fill(vm, ref, m, keys, vals)
    for oldest in (False, True):
        for k in sorted({0, max(live - 1, 0), live, live + 3}):
            check_order(lib, vm, ref, m, dev, k, oldest=oldest)
    check_lookup(vm, ref, m, np.concatenate([keys[::3], absent[:2]]), dev, f"{live} live: lookup")
    check_order(lib, vm, ref, m, dev, live, oldest=False)
    check_order(lib, vm, ref, m, dev, live // 2, oldest=True, evict=True)
    check_delete(vm, ref, m, np.concatenate([keys, absent[:1]]), dev, f"{live} live: delete everything")
    assert vm.map_count(m) == 0
    check_order(lib, vm, ref, m, dev, 4)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. lookup
def run_lookup(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(3)
    ks, vs, n = 13, 24, 200
    vm, ref, m, _ = lru_pair(lib, oracle_lib, ks, vs, 300)
    keys, vals, absent = entries(rng, ks, vs, n)
    fill(vm, ref, m, keys, vals)
    check_lookup(vm, ref, m, absent, dev, "absent keys only")
    check_lookup(vm, ref, m, np.repeat(keys[:40], 3, axis=0), dev, "every key three times in a row")
    check_lookup(vm, ref, m, np.tile(keys[10:60], (2, 1)), dev, "every key twice, a batch apart")
    check_lookup(vm, ref, m, np.repeat(keys[7:8], 257, axis=0), dev, "one key 257 times")
    # the promotion order: a shuffled batch with repetitions; the last occurrences decide
    batch = keys[rng.integers(0, n, size=150)]
    check_lookup(vm, ref, m, batch, dev, "promotion order")
    check_lookup(vm, ref, m, batch, dev, "promotion order", peek=True)
    # the host-pointer form
    hv, hf = vm.lru_lookup_batch(m, np.ascontiguousarray(batch[:65]))
    wv, wf = ref_lookup(ref, m, batch[:65], vs)
    assert np.array_equal(hv, wv) and np.array_equal(hf, wf)
    same_lru(vm, ref, m, "host-pointer lookup")
    vm.close()
    ref.close()


def run_chained(lib, oracle_lib, dev) -> None:
    """Device call after device call with no host read in between: every call works from the stamps and records
    the one before left (the links stay stale throughout); the oracle follows key by key, and the maps are
    compared at the end."""
    rng = np.random.default_rng(9)
    ks, vs, n = 8, 100, 280
    vm, ref, m, _ = lru_pair(lib, oracle_lib, ks, vs, 300)
    keys, vals, absent = entries(rng, ks, vs, n)
    fill(vm, ref, m, keys, vals)
    traffic = None
    for step in range(4):
        batch = np.ascontiguousarray(keys[rng.integers(0, n, size=65 + 64 * step)])
        gv, gf = vm.lru_lookup_batch(m, dev(batch))
        wv, wf = ref_lookup(ref, m, batch, vs)
        assert np.array_equal(to_np(gf), wf) and np.array_equal(to_np(gv), wv), f"step {step}: lookup"
        traffic = traffic or vm.map_traffic(m)
        gone = np.ascontiguousarray(np.concatenate([keys[rng.integers(0, n, size=9)], absent[:1]]))
        _, wf = ref_peek(ref, m, gone, vs)
        assert np.array_equal(to_np(vm.lru_delete_batch(m, dev(gone))), wf), f"step {step}: delete"
        for k in gone:
            ref.map_delete(m, k.tobytes())
        for oldest in (False, True):
            ek, ev, matched = expect_order(ref, m, None, oldest, 300)
            gk, gv, gm = call_order(lib, vm, m, dev, None, oldest, 300, 300)
            assert gm == matched and np.array_equal(gk, ek) and np.array_equal(gv, ev), f"step {step}: order, oldest {oldest}"
        ek, ev, matched = expect_order(ref, m, None, True, 11)
        gk, gv, gm = call_order(lib, vm, m, dev, None, True, 11, 11, evict=True)
        assert gm == matched and np.array_equal(gk, ek) and np.array_equal(gv, ev), f"step {step}: evict"
        for k in ek:
            ref.map_delete(m, k.tobytes())
    assert vm.map_traffic(m) == traffic, "a device call moved the whole map"
    same_lru(vm, ref, m, "after the chain")
    vm.close()
    ref.close()


def run_peek(lib, oracle_lib, dev) -> None:
    """XE_LRU_PEEK changes nothing and moves nothing; it is allowed inside a shard epoch, the promoting form
    is not."""
    rng = np.random.default_rng(5)
    vm, ref, m, _ = lru_pair(lib, oracle_lib, 4, 8, 300)
    keys, vals, absent = entries(rng, 4, 8, 100)
    fill(vm, ref, m, keys, vals)
    batch = np.ascontiguousarray(np.concatenate([keys[5:80], absent[:3], keys[5:9]]))
    check_lookup(vm, ref, m, batch[:9], dev, "the first call uploads", peek=True)
    order, dump, traffic = vm.map_lru_order(m), vm.map_dump(m), vm.map_traffic(m)
    for _ in range(2):
        vals_got, found = vm.lru_lookup_batch(m, dev(batch), peek=True)
        wv, wf = ref_peek(ref, m, batch, 8)
        assert np.array_equal(to_np(vals_got), wv) and np.array_equal(to_np(found), wf)
    check_order(lib, vm, ref, m, dev, 7)
    assert vm.map_traffic(m) == traffic, "a peek or an order moved the whole map"
    assert vm.map_lru_order(m) == order, "a peek changed the usage order"
    d2 = vm.map_dump(m)
    assert np.array_equal(d2[0], dump[0]) and np.array_equal(d2[1], dump[1])
    assert vm.map_traffic(m) == traffic, "the host reads after a peek downloaded the map again"
    # a promoting lookup moves nothing either, but the next host read downloads
    vm.lru_lookup_batch(m, dev(batch))
    ref_lookup(ref, m, batch, 8)
    assert vm.map_traffic(m) == traffic
    same_lru(vm, ref, m, "after a promoting lookup")
    assert vm.map_traffic(m) == (traffic[0], traffic[1] + 1)
    vm.close()
    ref.close()
    # inside a shard epoch (a VM with a program: the learning one over its LRU_HASH(4, 4, 64))
    vm, ref, m, _ = learn_vms(lib, oracle_lib, 40)
    batch = u32_keys([3, 39, 77, 3, 12, 1000, 0])
    vm.epoch_begin()
    vals_got, found = vm.lru_lookup_batch(m, dev(batch), peek=True)
    wv, wf = ref_peek(ref, m, batch, 4)
    assert np.array_equal(to_np(vals_got), wv) and np.array_equal(to_np(found), wf)
    assert rc_of(vm.lru_lookup_batch, m, dev(batch)) == ERR_INVAL
    assert rc_of(vm.lru_delete_batch, m, dev(batch)) == ERR_INVAL
    assert rc_of(vm.lru_evict, m, 3) == ERR_INVAL
    check_order(lib, vm, ref, m, dev, 5, oldest=True)
    vm.epoch_end()
    same_lru(vm, ref, m, "after the epoch")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 4. delete
def learn_vms(lib, oracle_lib, live: int, mode: int = 0):
    """The learning program of tests/test_lru_evict.py over an LRU_HASH(4, 4, 64) with `live` keys, twice."""
    import test_lru_evict as LE
    vm, ref = VM(Settings(engine=ENGINE_INTERP, mode=mode), lib=lib), VM(Settings(mode=mode), lib=oracle_lib)
    return vm, ref, LE._vm_setup(vm, LE._program(), LE.MAX, live), LE._vm_setup(ref, LE._program(), LE.MAX, live)


def same_batch(vm: VM, ref: VM, m: int, batch, what: str) -> None:
    umem, descs = batch
    a, b = vm.run_batch(umem.copy(), descs), ref.run_batch(umem.copy(), descs)
    assert (a.results == b.results).all(), f"{what}: results differ"
    assert np.array_equal(a.verdicts, b.verdicts), f"{what}: verdicts differ"
    same_lru(vm, ref, m, what)


def u32_keys(ids) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(ids, dtype=np.uint32)).view(np.uint8).reshape(-1, 4)


def run_delete(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(4)
    vm, ref, m, _ = lru_pair(lib, oracle_lib, 13, 100, 300)
    keys, vals, absent = entries(rng, 13, 100, 300)
    fill(vm, ref, m, keys, vals)
    check_delete(vm, ref, m, np.repeat(keys[:30], 4, axis=0), dev, "every key four times")
    check_delete(vm, ref, m, absent, dev, "absent keys only")
    check_delete(vm, ref, m, np.concatenate([keys[:30], keys[100:140], absent[:2], keys[100:140]]), dev, "deleted, present and absent keys")
    hf = vm.lru_delete_batch(m, np.ascontiguousarray(keys[140:150]))  # the host-pointer form
    for k in keys[140:150]:
        ref.map_delete(m, k.tobytes())
    assert list(hf) == [1] * 10
    same_lru(vm, ref, m, "host-pointer delete")
    check_lookup(vm, ref, m, keys[::5], dev, "lookup after the deletes")
    check_delete(vm, ref, m, keys, dev, "delete everything")
    assert vm.map_count(m) == 0
    check_lookup(vm, ref, m, keys[:5], dev, "lookup in the emptied map")
    vm.close()
    ref.close()


def run_delete_then_learn(lib, oracle_lib, dev) -> None:
    """Keys deleted on the device are inserted again by a batch run (through the tombstones the delete left)."""
    import test_lru_evict as LE
    vm, ref, m, _ = learn_vms(lib, oracle_lib, LE.MAX)
    gone = u32_keys([3, 4, 5, 40, 41, 63])
    check_delete(vm, ref, m, gone, dev, "delete before the batch")
    n = 24
    ids = np.tile(np.array([3, 4, 5, 40, 41, 63], dtype=np.uint32), 4)
    same_batch(vm, ref, m, LE._batch(np.ones(n, dtype=np.uint32), ids), "re-insert of deleted keys")
    check_lookup(vm, ref, m, u32_keys(range(0, 64, 3)), dev, "lookup after the re-insert")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 5. order / evict
VS_F = 24
FILTER_FIELDS = ((8, 8), (3, 2))  # (offset, width): an aligned 8-byte field and an unaligned 2-byte one


def filter_map(lib, oracle_lib, n: int = 200):
    """Values whose two filter fields take few distinct values, so every op selects a proper subset."""
    rng = np.random.default_rng(6)
    vm, ref, m, _ = lru_pair(lib, oracle_lib, 13, VS_F, 300)
    keys, vals, _ = entries(rng, 13, VS_F, n)
    vals[:, 8:16] = (rng.integers(0, 6, size=n).astype(np.uint64) * np.uint64(0x0101010101010101)).view(np.uint8).reshape(-1, 8)
    vals[:, 3:5] = rng.integers(0, 6, size=n).astype(np.uint16).view(np.uint8).reshape(-1, 2)
    fill(vm, ref, m, keys, vals)
    return vm, ref, m, keys


def filters():
    out = []
    for off, width in FILTER_FIELDS:
        unit = 0x0101010101010101 if width == 8 else 1
        for op in OPS:
            out.append(None if op == ALL else MapFilter(op, off, width, 3 * unit))
    return out


def run_order(lib, oracle_lib, dev, evict: bool = False) -> None:
    vm, ref, m, keys = filter_map(lib, oracle_lib)
    for i, flt in enumerate(filters()):
        matched = expect_order(ref, m, flt, False, 0)[2]
        assert evict or flt is None or 0 < matched < vm.map_count(m), "the filter selects a proper subset"
        for oldest in (False, True):
            # k = 0, below, at and above matched; an evict takes at most two a call, so the map lasts the matrix
            ks = (0, min(matched, 2)) if evict else sorted({0, 1, max(matched - 1, 0), matched, matched + 5})
            for k in ks:
                check_order(lib, vm, ref, m, dev, k, flt=flt, oldest=oldest, evict=evict, host_form=bool(i & 1))
    flt = MapFilter(NE, 3, 2, 3)
    if evict:  # at and above matched
        matched = expect_order(ref, m, flt, False, 0)[2]
        check_order(lib, vm, ref, m, dev, matched // 2, flt=flt, oldest=False, evict=True)
        check_order(lib, vm, ref, m, dev, matched - matched // 2, flt=flt, oldest=True, evict=True)
        check_order(lib, vm, ref, m, dev, 5, flt=flt, oldest=True, evict=True)
    flt = MapFilter(EQ, 8, 8, 0)
    check_order(lib, vm, ref, m, dev, 9, flt=flt, oldest=True, evict=evict, want_keys=False)
    check_order(lib, vm, ref, m, dev, 9, flt=flt, oldest=False, evict=evict, want_vals=False)
    check_order(lib, vm, ref, m, dev, 9, oldest=True, evict=evict, koff=1, voff=3)
    if evict:  # nothing to report, still removed
        ek, _, _ = expect_order(ref, m, None, True, 6)
        rc, matched = raw_order(lib, vm, m, None, OLDEST, 0, 0, 6, evict=True)
        assert rc == 0 and matched == ref.map_count(m)
        for kk in ek:
            ref.map_delete(m, kk.tobytes())
        same_lru(vm, ref, m, "evict with neither output")
    # the whole map, most recent first: byte for byte what xe_map_lru_order writes
    n = ref.map_count(m)
    gk, _, gm = call_order(lib, vm, m, dev, None, False, n + 10, n + 10)
    assert gm == n and gk.tobytes() == b"".join(ref.map_lru_order(m))
    same_lru(vm, ref, m, "after the orders")
    vm.close()
    ref.close()


def nil_vms(lib, oracle_lib):
    """The program and packets of tests/test_lru_nil_value.py: three of the four keys of an LRU_HASH(4, 8, 16) end
    nil-backed."""
    from parity import packets
    from test_lru_nil_value import _program
    umem, descs = packets(600, 64, seed=9)
    for d in descs:
        umem[int(d["addr"]) + 1] = 0
    for i in (150, 151, 400):
        umem[int(descs[i]["addr"]) + 1] = 1
    out = []
    for lb in (lib, oracle_lib):
        vm = VM(Settings(engine=ENGINE_INTERP), lib=lb)
        m = vm.add_map(MapDef(MAP_LRU_HASH, 4, 8, 16))
        vm.set_entrypoint(vm.add_raw_program(_program()))
        out.append((vm, vm.run_batch(umem.copy(), descs)))
    (vm, got), (ref, want) = out
    assert np.array_equal(got.verdicts, want.verdicts)
    return vm, ref, m


def run_nil_backed(lib, oracle_lib, dev) -> None:
    vm, ref, m = nil_vms(lib, oracle_lib)
    keys = u32_keys([0, 1, 2, 3, 77])
    wv, wf = ref_peek(ref, m, keys, 8)
    assert list(wf) == [1, 1, 1, 1, 0] and int((~wv[:4].any(axis=1)).sum()) == 3, "the batch left no nil-backed values"
    check_lookup(vm, ref, m, keys, dev, "peek at nil-backed values", peek=True)
    for flt in (None, MapFilter(EQ, 0, 8, 0), MapFilter(NE, 0, 8, 0)):  # a nil-backed value reads as zeros
        for oldest in (False, True):
            check_order(lib, vm, ref, m, dev, 4, flt=flt, oldest=oldest)
    check_lookup(vm, ref, m, keys, dev, "lookup of nil-backed values")
    check_order(lib, vm, ref, m, dev, 2, flt=MapFilter(EQ, 0, 8, 0), oldest=True, evict=True)
    check_delete(vm, ref, m, keys, dev, "delete of nil-backed values")
    vm.close()
    ref.close()


def run_evict_then_learn(lib, oracle_lib, dev, mode: int = 0) -> None:
    """Evict the k oldest of a full map, then a learning batch that fills it again and evicts on its own: verdicts,
    the dump and the usage order equal the oracle's, where the same keys were deleted one by one."""
    import test_lru_evict as LE
    vm, ref, m, _ = learn_vms(lib, oracle_lib, LE.MAX, mode)
    assert check_order(lib, vm, ref, m, dev, 20, oldest=True, evict=True) == 20
    assert vm.map_count(m) == LE.MAX - 20
    same_batch(vm, ref, m, LE._learning_batch(400, 1), "a learning batch after the evict")
    assert vm.map_count(m) == LE.MAX
    check_order(lib, vm, ref, m, dev, 7, oldest=True, evict=True)
    same_batch(vm, ref, m, LE._learning_batch(300, 2), "a second batch")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 6. state the kernels did not create
def run_state(lib, oracle_lib, dev, state: str) -> None:
    import test_lru_evict as LE
    mode = MODE_SEQUENTIAL if state == "one_lane_replay" else 0
    vm, ref, m, _ = learn_vms(lib, oracle_lib, LE.MAX - 10, mode)
    if state == "epoch_wrap":  # the batch's stamps carry the last epoch; the lookup's own must renumber first
        assert lib.debug_set_lru_epoch(vm.h, 0xfffe) == 0
    if state != "fresh_upload":
        umem, descs = LE._learning_batch(400, 5, live=LE.MAX - 10)
        a, b = vm.run_batch(umem.copy(), descs), ref.run_batch(umem.copy(), descs)
        assert (a.results == b.results).all()
        if state == "one_lane_replay":
            assert a.stats["mode_used"] == MODE_SEQUENTIAL
    for oldest in (False, True):
        check_order(lib, vm, ref, m, dev, LE.MAX, oldest=oldest)
    live = ref.map_lru_order(m)
    batch = np.frombuffer(b"".join(live[::-2] + live[:5]), dtype=np.uint8).reshape(-1, 4)
    vals, found = vm.lru_lookup_batch(m, dev(np.ascontiguousarray(batch)))
    wv, wf = ref_lookup(ref, m, batch, 4)
    assert np.array_equal(to_np(found), wf) and np.array_equal(to_np(vals), wv)
    for oldest in (False, True):  # from the stamps alone, before any host read relinks
        check_order(lib, vm, ref, m, dev, LE.MAX, oldest=oldest)
    same_lru(vm, ref, m, f"{state}: after the promoting lookup")
    check_order(lib, vm, ref, m, dev, 5, oldest=True, evict=True)
    same_batch(vm, ref, m, LE._learning_batch(200, 6, live=LE.MAX - 10), f"{state}: a batch afterwards")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 7. errors
def run_errors(lib, dev) -> None:
    k, v, f = np.zeros((2, 4), np.uint8), np.zeros((2, 8), np.uint8), np.zeros(2, np.uint8)
    kp, vp, fp = k.ctypes.data, v.ctypes.data, f.ctypes.data
    n = C.c_uint64(7)
    vm = VM(Settings(engine=ENGINE_INTERP), lib=lib)
    h = vm.add_map(MapDef(MAP_HASH, 4, 8, 16))
    # a map that is not LRU_HASH, as xe_map_lru_order
    assert lib.map_lru_order(vm.h, h, None, 0, C.byref(n)) == ERR_INVAL
    assert lib.lru_lookup_batch_device(vm.h, h, kp, 2, vp, fp, 0, None) == ERR_INVAL
    assert lib.lru_lookup_batch_device(vm.h, h, kp, 2, vp, fp, PEEK, None) == ERR_INVAL
    assert lib.lru_delete_batch_device(vm.h, h, kp, 2, fp, None) == ERR_INVAL
    assert lib.lru_order_device(vm.h, h, None, 0, kp, vp, 2, C.byref(n), None) == ERR_INVAL
    assert lib.lru_evict_device(vm.h, h, None, 0, kp, vp, 2, C.byref(n), None) == ERR_INVAL
    assert lib.lru_lookup_batch(vm.h, h, kp, 2, vp, fp, 0) == ERR_INVAL
    assert lib.lru_delete_batch(vm.h, h, kp, 2, fp) == ERR_INVAL
    assert lib.lru_order(vm.h, h, None, 0, kp, vp, 2, C.byref(n)) == ERR_INVAL
    assert lib.lru_evict(vm.h, h, None, 0, kp, vp, 2, C.byref(n)) == ERR_INVAL
    assert lib.lru_order_device(vm.h, 99, None, 0, kp, vp, 2, C.byref(n), None) == ERR_INVAL
    m = vm.add_map(MapDef(MAP_LRU_HASH, 4, 8, 16))
    vm.map_update(m, b"\1\0\0\0", b"\7" * 8)
    # NULL matched, NULL required pointers, too many keys
    for fn in (lib.lru_order_device, lib.lru_evict_device):
        assert fn(vm.h, m, None, 0, kp, vp, 2, None, None) == ERR_INVAL
    for fn in (lib.lru_order, lib.lru_evict):
        assert fn(vm.h, m, None, 0, kp, vp, 2, None) == ERR_INVAL
    assert lib.lru_lookup_batch_device(vm.h, m, None, 2, vp, fp, 0, None) == ERR_INVAL
    assert lib.lru_lookup_batch_device(vm.h, m, kp, 2, None, fp, 0, None) == ERR_INVAL
    assert lib.lru_delete_batch_device(vm.h, m, None, 2, fp, None) == ERR_INVAL
    assert lib.lru_lookup_batch_device(vm.h, m, kp, (1 << 31) + 1, vp, fp, PEEK, None) == ERR_INVAL
    assert lib.lru_delete_batch_device(vm.h, m, kp, (1 << 31) + 1, fp, None) == ERR_INVAL
    assert lib.lru_lookup_batch_device(vm.h, m, None, 0, None, None, 0, None) == 0  # count 0: nothing to do
    # unknown flag bits
    assert lib.lru_lookup_batch_device(vm.h, m, kp, 2, vp, fp, 2, None) == ERR_INVAL
    assert lib.lru_lookup_batch(vm.h, m, kp, 2, vp, fp, 3) == ERR_INVAL
    for fn in (lib.lru_order_device, lib.lru_evict_device):
        assert fn(vm.h, m, None, 2, kp, vp, 2, C.byref(n), None) == ERR_INVAL
    for fn in (lib.lru_order, lib.lru_evict):
        assert fn(vm.h, m, None, 0x80000001, kp, vp, 2, C.byref(n)) == ERR_INVAL
    # the scan's filter errors, unchanged
    bad = (N.MapFilter(9, 0, 8, 0, 0), N.MapFilter(EQ, 0, 3, 0, 0), N.MapFilter(EQ, 1, 8, 0, 0), N.MapFilter(EQ, 8, 1, 0, 0),
           N.MapFilter(EQ, 0, 8, 1, 0), N.MapFilter(EQ, 0xffffffff, 8, 0, 0))
    for flt in bad:
        for evict in (False, True):
            for device_form in (False, True):
                assert raw_order(lib, vm, m, flt, 0, kp, vp, 2, device_form, evict)[0] == ERR_INVAL, (flt.op, flt.offset, flt.width)
    assert vm.map_count(m) == 1 and vm.map_lookup(m, b"\1\0\0\0") == b"\7" * 8, "a refused call changed the map"
    # the calls for ARRAY and HASH maps keep refusing an LRU map
    flt, order = N.MapFilter(), N.MapOrder(0, 8, 0, 0)
    assert lib.map_lookup_batch_device(vm.h, m, kp, 2, vp, fp, None) == ERR_UNSUPPORTED
    assert b"ARRAY and HASH" in lib.last_error(vm.h)
    assert lib.map_delete_batch_device(vm.h, m, kp, 2, fp, None) == ERR_UNSUPPORTED
    assert lib.map_update_batch_device(vm.h, m, kp, vp, 2, None) == ERR_UNSUPPORTED
    assert lib.map_scan_device(vm.h, m, C.byref(flt), kp, vp, 2, C.byref(n), None) == ERR_UNSUPPORTED
    assert lib.map_expire_device(vm.h, m, C.byref(flt), kp, vp, 2, C.byref(n), None) == ERR_UNSUPPORTED
    assert lib.map_top_device(vm.h, m, None, C.byref(order), kp, vp, 2, C.byref(n), None, None) == ERR_UNSUPPORTED
    assert lib.map_evict_device(vm.h, m, None, C.byref(order), kp, vp, 2, C.byref(n), None, None) == ERR_UNSUPPORTED
    info = N.MapCompactInfo()
    assert lib.map_compact(vm.h, m, 0, C.byref(info), None) == ERR_UNSUPPORTED
    vm.close()


# ---------------------------------------------------------------- 8. the Python interface
def run_python_api(lib, oracle_lib, dev, on_device: bool) -> None:
    rng = np.random.default_rng(8)
    vm, ref, m, _ = lru_pair(lib, oracle_lib, 8, 24, 64)
    keys, vals, absent = entries(rng, 8, 24, 50)
    fill(vm, ref, m, keys, vals)
    mk = dev if on_device else np.ascontiguousarray
    batch = np.ascontiguousarray(np.concatenate([keys[10:20], absent[:2]]))
    gv, gf = vm.lru_lookup_batch(m, mk(batch))
    wv, wf = ref_lookup(ref, m, batch, 24)
    assert np.array_equal(to_np(gv), wv) and np.array_equal(to_np(gf), wf)
    for oldest in (False, True):
        ek, ev, matched = expect_order(ref, m, None, oldest, 12)
        gk, gv, gm = vm.lru_order(m, 12, oldest_first=oldest, on_device=on_device)
        assert gm == matched and np.array_equal(to_np(gk), ek) and np.array_equal(to_np(gv), ev)
    ek, ev, matched = expect_order(ref, m, None, True, 5)
    gk, gv, gm = vm.lru_evict(m, 5, on_device=on_device)
    assert gm == matched and np.array_equal(to_np(gk), ek) and np.array_equal(to_np(gv), ev)
    for kk in ek:
        ref.map_delete(m, kk.tobytes())
    found = vm.lru_delete_batch(m, mk(batch))
    _, wf = ref_peek(ref, m, batch, 24)
    for kk in batch:
        ref.map_delete(m, kk.tobytes())
    assert np.array_equal(to_np(found), wf)
    same_lru(vm, ref, m, "the Python interface")
    try:
        vm.lru_order(vm.add_map(MapDef(MAP_HASH, 4, 8, 16)), 3)
        raise AssertionError("a HASH map was accepted")
    except EmulatorError as e:
        assert e.rc == ERR_INVAL
    vm.close()
    ref.close()
