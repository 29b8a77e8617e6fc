"""Shared cases of the device-side top-K, evict and value statistics (xe_map_top_device,
xe_map_evict_device, xe_map_stats and the host-pointer forms): tests/test_maptop.py runs them on the host
simulation, tests/test_maptop_gpu.py on the product library.

No expected value comes from the code under test:
  * the eligible entries are a mapscan_cases.Snapshot (the oracle's dump as a set, the exported state
    image for the slot order), filtered by mapscan_cases.selects;
  * the rank is np.lexsort((slot position, field or ~field)): by the field in the asked direction, ties in
    slot order; the first r = min(k, matched) of it, sorted by slot again, are the exact keys and values a
    call must write; matched and cut follow from the same arrays. The restatement is pinned by RANK_TABLE,
    worked out by hand;
  * statistics are Python integers over the same arrays;
  * after an evict the oracle deletes the same keys one by one and the maps are compared as
    mapscan_cases.check_expire compares them.

`dev` is mapscan_cases': a numpy array stays one on the host simulation and becomes a CUDA tensor on the
product; host_form sends a call through the host-pointer forms.

Sizes (xe_mapops.h): a tile is 256 slots in 4 rounds of 64, so the k of run_ties cut inside a round, at a
round's edge and at a tile's edge; the SCAN step takes 1,024 tile counts a pass, so the 2^20-slot table of
SLOT_CASES makes both SCANs of a call carry; a histogram bin is a u32 flushed from LDS, and the 4,099-entry
ARRAY cases put more than 2^12 entries into one bin."""
from __future__ import annotations

import ctypes as C

import numpy as np

import mapops_cases as MC
import mapscan_cases as SC
from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, VM, MapDef,
                                  MapFilter, MapOrder, Settings)
from mapops_cases import (GUARD, addr, flow_vm, guards_intact, hash_pool, image_records, on_dev, pair, place, same_image_map,
                          same_map, settle, state_image, to_np, Runner)
from mapscan_cases import ALL, ANYBITS, EQ, GE, GT, M64, NE, OPS, Snapshot, fields, fill_hash, selects

WIDTHS = (1, 2, 4, 8)
SHAPE_PAIRS = ((0, 24), (8, 8), (13, 17), (24, 65), (56, 1024), (64, 4096))
WIDTH_VALUE_SIZES = (9, 17, 65, 1025)
ALIGN_OFFSETS = (0, 1, 4, 8)


# ---------------------------------------------------------------- the rank, restated
def rank_positions(f: np.ndarray, descending: bool, k: int):
    """f: the order fields (uint64) of the eligible entries in slot order. Returns (the positions of the
    first min(k, len) entries of the rank, ascending; the field of the last of them, or 0)."""
    f = np.asarray(f, dtype=np.uint64)
    order = np.lexsort((np.arange(len(f)), ~f if descending else f))
    r = min(k, len(f))
    return np.sort(order[:r]), (int(f[order[r - 1]]) if r else 0)


B63 = 1 << 63
# (fields in slot order, descending, k, selected positions, cut), worked out by hand
RANK_TABLE = (
    ((5, 9, 5, 1), True, 1, (1,), 9),
    ((5, 9, 5, 1), True, 2, (0, 1), 5),          # the tie goes to the earlier slot
    ((5, 9, 5, 1), True, 3, (0, 1, 2), 5),
    ((5, 9, 5, 1), False, 1, (3,), 1),
    ((5, 9, 5, 1), False, 2, (0, 3), 5),
    ((5, 9, 5, 1), False, 9, (0, 1, 2, 3), 9),   # k past the entries
    ((5, 9, 5, 1), True, 9, (0, 1, 2, 3), 1),
    ((5, 9, 5, 1), True, 0, (), 0),
    ((), False, 3, (), 0),
    ((7, 7, 7, 7), True, 2, (0, 1), 7),
    ((7, 7, 7, 7), False, 3, (0, 1, 2), 7),
    ((1, B63, B63 - 1, B63 | 1), True, 1, (3,), B63 | 1),   # bit 63 set: unsigned
    ((1, B63, B63 - 1, B63 | 1), True, 2, (1, 3), B63),
    ((1, B63, B63 - 1, B63 | 1), True, 3, (1, 2, 3), B63 - 1),
    ((1, B63, B63 - 1, B63 | 1), False, 2, (0, 2), B63 - 1),
    ((1, B63, B63 - 1, B63 | 1), False, 3, (0, 1, 2), B63),
    ((M64, 0, M64), True, 1, (0,), M64),
    ((M64, 0, M64), False, 1, (1,), 0),
    ((M64, 0, M64), False, 2, (0, 1), M64),
)


def check_rank_table() -> None:
    for f, desc, k, want, cut in RANK_TABLE:
        got, gcut = rank_positions(np.array(f, dtype=np.uint64), desc, k)
        assert tuple(int(x) for x in got) == want and gcut == cut, (f, desc, k, got, gcut)


def expect_top(snap: Snapshot, flt, order: MapOrder, k: int):
    """(keys, values, matched, cut, positions in the snapshot) a call must report."""
    snap.expect(flt)  # the eligible set is the oracle's
    pos = np.nonzero(selects(snap.vals, flt))[0]
    f = fields(snap.vals[pos], order.offset, order.width)
    chosen, cut = rank_positions(f, bool(order.descending), k)
    at = pos[chosen]
    return snap.keys[at], snap.vals[at], len(pos), cut, at


def expect_stats(snap: Snapshot, flt, field: MapOrder) -> dict:
    snap.expect(flt)
    f = [int(x) for x in fields(snap.vals[selects(snap.vals, flt)], field.offset, field.width)]
    return {"count": len(f), "sum": sum(f) & M64, "min": min(f) if f else M64, "max": max(f) if f else 0}


# ---------------------------------------------------------------- the calls
def c_filter(flt):
    return None if flt is None else (flt if isinstance(flt, N.MapFilter) else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand))


def c_order(order):
    return None if order is None else (order if isinstance(order, N.MapOrder) else
                                       N.MapOrder(order.offset, order.width, int(order.descending), 0))


def raw_top(lib, vm: VM, m: int, flt, order, kptr, vptr, k: int, device_form: bool, evict: bool = False, matched=True, cut=True):
    """One call by address. Returns (rc, matched, cut)."""
    cf, co = c_filter(flt), c_order(order)
    n, c = C.c_uint64(0xDEADBEEF), C.c_uint64(0xDEADBEEF)
    head = (vm.h, m, None if cf is None else C.byref(cf), None if co is None else C.byref(co), kptr or None, vptr or None, k,
            C.byref(n) if matched else None, C.byref(c) if cut else None)
    if device_form:
        rc = (lib.map_evict_device if evict else lib.map_top_device)(*head, None)
    else:
        rc = (lib.map_evict if evict else lib.map_top)(*head)
    return rc, n.value, c.value


def raw_stats(lib, vm: VM, m: int, flt, field, out=True):
    cf, co, st = c_filter(flt), c_order(field), N.MapStats(1, 2, 3, 4)
    rc = lib.map_stats(vm.h, m, None if cf is None else C.byref(cf), None if co is None else C.byref(co),
                       C.byref(st) if out else None, None)
    return rc, {"count": st.count, "sum": st.sum, "min": st.min, "max": st.max}


def call(lib, vm: VM, m: int, dev, flt, order, k: int, room: int, evict: bool = False, koff: int = 0, voff: int = 0,
         want_keys: bool = True, want_vals: bool = True, host_form: bool = False, want_cut: bool = True):
    """A top or an evict into GUARD buffers of `room` entries, koff / voff bytes past a 16-byte boundary.
    Returns (keys[r], values[r], matched, cut, the two whole buffers) after checking that no byte in front of
    the buffers or behind entry r was written."""
    d = vm.map_defs[m]
    ks, vs = (4 if d.type == MAP_ARRAY else d.key_size), d.value_size
    mk = np.ascontiguousarray if host_form else dev
    kbuf, _ = place(mk, np.full((room, ks), GUARD, np.uint8), koff)
    vbuf, _ = place(mk, np.full((room, vs), GUARD, np.uint8), voff)
    settle(kbuf)
    settle(vbuf)
    rc, matched, cut = raw_top(lib, vm, m, flt, order, addr(kbuf) + koff if want_keys else 0, addr(vbuf) + voff if want_vals else 0,
                               k, not host_form, evict, cut=want_cut)
    assert rc == 0, lib.last_error(vm.h)
    r = min(matched, k)
    assert r <= room
    what = f"{'evict' if evict else 'top'} k {k}, keys +{koff}, values +{voff}"
    kk = guards_intact(kbuf, koff, r * ks if want_keys else 0, what + ": keys")
    kk = kk.reshape(-1, ks) if ks else np.zeros((r, 0), np.uint8)
    v = guards_intact(vbuf, voff, r * vs if want_vals else 0, what + ": values").reshape(-1, vs)
    return kk, v, matched, cut, (to_np(kbuf).copy(), to_np(vbuf).copy())


def check_top(lib, vm, snap: Snapshot, m, dev, order: MapOrder, k: int, flt=None, **kw):
    ek, ev, matched, cut, at = expect_top(snap, flt, order, k)
    gk, gv, gm, gc, _ = call(lib, vm, m, dev, flt, order, k, len(ek) + 3, **kw)
    what = f"top k {k} order {order} filter {flt}"
    assert gm == matched, f"{what}: matched {gm}, expected {matched}"
    if kw.get("want_cut", True):
        assert gc == cut, f"{what}: cut {gc:#x}, expected {cut:#x}"
    if kw.get("want_keys", True):
        assert np.array_equal(gk, ek), f"{what}: keys differ (or their order)"
    if kw.get("want_vals", True):
        assert np.array_equal(gv, ev), f"{what}: values differ (or their order)"
    return ek, ev, matched, cut


def check_stats(lib, vm, snap: Snapshot, m, field: MapOrder, flt=None) -> dict:
    want = expect_stats(snap, flt, field)
    rc, got = raw_stats(lib, vm, m, flt, field)
    assert rc == 0, lib.last_error(vm.h)
    assert got == want, f"stats of {field} under {flt}: {got}, expected {want}"
    return want


def check_evict(lib, vm, ref, m, dev, order: MapOrder, k: int, flt=None, host_visit: bool = True, **kw):
    """An evict against the state before it; then the oracle deletes the same keys one by one and the maps
    must agree as after an expire. Returns (the evicted keys, the snapshot before)."""
    before = Snapshot(vm, ref, m, dev)
    ek, ev, matched, cut, at = expect_top(before, flt, order, k)
    r = len(ek)
    gk, gv, gm, gc, _ = call(lib, vm, m, dev, flt, order, k, r + 3, evict=True, **kw)
    assert (gm, gc) == (matched, cut), f"evict k {k}: matched {gm} cut {gc:#x}, expected {matched} {cut:#x}"
    if kw.get("want_keys", True):
        assert np.array_equal(gk, ek), "keys differ (or their order)"
    if kw.get("want_vals", True):
        assert np.array_equal(gv, ev), "values differ: the values before the removal are reported"
    MC.ref_delete(ref, m, ek)
    img = same_image_map(vm, ref, m, dev, "after the evict")
    w0, keys, vals, count = image_records(vm, m, img)
    gone = before.slots[at]
    assert (w0[gone] == np.uint64(MC.SLOT_TOMB)).all(), "a removed record is not a plain tombstone"
    assert np.array_equal(keys[gone], ek), "a removed record lost its key words"
    assert not vals[gone].any(), "a removed record's value is not zero"
    assert count == len(before.keys) - r
    assert int(((w0 & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == before.tombs + r
    if host_visit:
        same_map(vm, ref, m, "after the evict")
        assert vm.map_count(m) == ref.map_count(m) == len(before.keys) - r
    return ek, before


def ks_around(matched: int):
    return (1, 63, 64, 65, 255, 256, 257, matched - 1, matched, matched + 5)


# ---------------------------------------------------------------- 1. ties across the boundaries
def run_ties_hash(lib, oracle_lib, dev, host_form: bool = False) -> None:
    rng = np.random.default_rng(101)
    ks, vs, n = 8, 16, 900
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 1024))
    keys = hash_pool(rng, ks, n)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    vals[:, 4:12] = np.frombuffer((0x8000000000123456).to_bytes(8, "little"), np.uint8)  # every order field equal
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, m, keys, vals)
    gone = np.ascontiguousarray(keys[::3])
    assert to_np(vm.map_delete_batch(m, dev(gone))).all()
    MC.ref_delete(ref, m, gone)
    snap = Snapshot(vm, ref, m, dev)
    live = len(snap.keys)
    assert live == 600 and snap.tombs == 300
    for i, k in enumerate(ks_around(live)):
        ek, _, matched, cut = check_top(lib, vm, snap, m, dev, MapOrder(4, 8, i % 2 == 0), k, host_form=host_form)
        assert matched == live and cut == 0x8000000000123456
        assert np.array_equal(ek, snap.keys[:min(k, live)])  # what the case names: the first k in slot order
    vm.close()
    ref.close()


def run_ties_array(lib, oracle_lib, dev, host_form: bool = False) -> None:
    entries, vs = 4099, 8
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, entries))
    idx = np.arange(0, entries, 5, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vals = np.zeros((len(idx), vs), np.uint8)
    vals[:, 0] = np.arange(len(idx)) % 251 + 1  # byte 0 is not part of the order field
    vm.map_update_batch_device(m, dev(idx), dev(vals))
    MC.ref_update(ref, m, idx, vals)
    snap = Snapshot(vm, ref, m, dev)
    for i, k in enumerate(ks_around(entries)):
        ek, _, matched, cut = check_top(lib, vm, snap, m, dev, MapOrder(1, 4, i % 2 == 1), k, host_form=host_form)
        assert matched == entries and cut == 0
        assert np.array_equal(ek.view(np.uint32).reshape(-1), np.arange(min(k, entries), dtype=np.uint32))
    # ... and among a filter's matches
    flt = MapFilter(NE, 0, 1, 0)
    ek, _, matched, _ = check_top(lib, vm, snap, m, dev, MapOrder(1, 4, True), 300, flt, host_form=host_form)
    assert matched == len(idx) and np.array_equal(ek, idx[:300])
    same_map(vm, ref, m, "ARRAY after the tops")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. digit order
def run_digits(lib, oracle_lib, dev, byte: int, host_form: bool = False) -> None:
    """A width-8 field whose values differ in one byte only (six distinct values in runs; for byte 7 some
    have bit 63 set), both directions, k inside a run of equal values and exactly at its edge."""
    rng = np.random.default_rng(200 + byte)
    ks, vs, n = 8, 16, 300
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 512))
    keys = hash_pool(rng, ks, n)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    base = 0x0102030405060708 & ~(0xff << (8 * byte))
    digits = np.array([0x00, 0x01, 0x7f, 0x80, 0xfe, 0xff], dtype=np.uint64)[rng.integers(0, 6, size=n)]
    f = np.uint64(base) | (digits << np.uint64(8 * byte))
    vals[:, 3:11] = f.view(np.uint8).reshape(n, 8)
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, m, keys, vals)
    snap = Snapshot(vm, ref, m, dev)
    got = fields(snap.vals, 3, 8)
    assert len(np.unique(got)) == 6 and (byte != 7 or (got >> np.uint64(63)).any())
    for desc in (True, False):
        order = MapOrder(3, 8, desc)
        runs = np.sort(got)[::-1] if desc else np.sort(got)
        edges = [int(e) + 1 for e in np.nonzero(runs[1:] != runs[:-1])[0]]  # the lengths of the first 1 .. 5 runs
        assert len(edges) == 5 and edges[0] >= 3
        for k in (edges[0] - 1, edges[0], edges[0] + 1, edges[2], edges[4] - 1, edges[4] + 1, n):
            _, _, matched, cut = check_top(lib, vm, snap, m, dev, order, k, host_form=host_form)
            assert matched == n and cut == int(runs[k - 1])
    vm.close()
    ref.close()


def run_one_bin(lib, oracle_lib, dev) -> None:
    """4,099 entries that share the seven high bytes of the field (bit 63 set): one histogram bin holds
    more than 2^12 entries in seven of the eight passes."""
    entries, vs = 4099, 9
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, entries))
    idx = np.arange(entries, dtype=np.uint32)
    f = np.uint64(0x80ffee0000000000) | ((idx.astype(np.uint64) * np.uint64(37)) % np.uint64(11))
    vals = np.zeros((entries, vs), np.uint8)
    vals[:, 1:9] = f.view(np.uint8).reshape(entries, 8)
    vm.map_update_batch_device(m, dev(idx.view(np.uint8).reshape(-1, 4)), dev(vals))
    MC.ref_update(ref, m, idx.view(np.uint8).reshape(-1, 4), vals)
    snap = Snapshot(vm, ref, m, dev)
    for desc, k in ((True, 1), (True, 372), (True, 373), (False, 374), (False, 4098), (True, 5000)):
        _, _, matched, cut = check_top(lib, vm, snap, m, dev, MapOrder(1, 8, desc), k)
        assert matched == entries and cut >> 40 == 0x80ffee
    check_stats(lib, vm, snap, m, MapOrder(1, 8))
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. widths and offsets
def run_widths(lib, oracle_lib, dev, vs: int, host_form: bool = False) -> None:
    rng = np.random.default_rng(300 + vs)
    ks, n = 8, 60
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, n)
    snap = Snapshot(vm, ref, m, dev)
    i = 0
    for width in WIDTHS:
        for off in sorted(o for o in {0, 1, 3, vs - width} if o + width <= vs):  # (9-byte values: no 8-byte field at +3)
            fo = off - 1 if off else off + width  # the filter looks at a byte outside the order field
            assert fo < vs and not (off <= fo < off + width)
            flt = MapFilter(ANYBITS, fo, 1, 1)
            order = MapOrder(off, width, i % 2 == 0)
            _, _, matched, _ = check_top(lib, vm, snap, m, dev, order, 7, flt, host_form=host_form)
            assert 8 <= matched < len(snap.keys)
            check_top(lib, vm, snap, m, dev, order, matched - 1, flt, host_form=host_form)
            check_stats(lib, vm, snap, m, order, flt)
            i += 1
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 4. filter interplay
def run_filters(lib, oracle_lib, dev, host_form: bool = False) -> None:
    rng = np.random.default_rng(404)
    ks, vs, n = 13, 24, 60
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, n)
    snap = Snapshot(vm, ref, m, dev)
    live = len(snap.keys)
    order = MapOrder(9, 4, True)
    operand = int(fields(snap.vals, 16, 8)[live // 2])
    count = {}
    for op in OPS:
        flt = MapFilter(op, 16, 8, operand)
        for k in (5, live):
            count[op] = check_top(lib, vm, snap, m, dev, order, k, flt, host_form=host_form)[2]
        check_stats(lib, vm, snap, m, order, flt)
    assert count[ALL] == live and count[EQ] == 1 and count[NE] == live - 1 and count[GE] + count[SC.LT] == live
    # a filter selecting one entry
    ek, _, matched, cut = check_top(lib, vm, snap, m, dev, MapOrder(9, 4, False), 3, MapFilter(EQ, 16, 8, operand), host_form=host_form)
    assert matched == 1 and len(ek) == 1
    # a filter selecting nothing: no byte written, cut 0; an evict changes nothing
    none = MapFilter(GT, 0, 1, 0xfff)
    ek, _, matched, cut = check_top(lib, vm, snap, m, dev, order, 5, none, host_form=host_form)
    assert (len(ek), matched, cut) == (0, 0, 0)
    assert check_stats(lib, vm, snap, m, order, none) == {"count": 0, "sum": 0, "min": M64, "max": 0}
    before = state_image(vm, m, dev)
    gk, gv, gm, gc, _ = call(lib, vm, m, dev, none, order, 5, 4, evict=True, host_form=host_form)
    assert (len(gk), gm, gc) == (0, 0, 0)
    assert np.array_equal(before, state_image(vm, m, dev)), "an evict of nothing changed the map"
    same_map(vm, ref, m, "after an evict of nothing")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 5. key and value shapes
def run_shape(lib, oracle_lib, dev, ks: int, vs: int, host_form: bool = False) -> None:
    if ks == 0:
        return run_empty_key(lib, oracle_lib, dev, vs, host_form)
    rng = np.random.default_rng(5000 * ks + vs)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    fill_hash(vm, ref, m, dev, rng, ks, vs, MC.HASH_MAX // 2)
    snap = Snapshot(vm, ref, m, dev)
    assert len(snap.keys) == 21
    w = SC.widest(vs)
    for desc in (True, False):
        for k in (5, 21):
            check_top(lib, vm, snap, m, dev, MapOrder(vs - w, w, desc), k, host_form=host_form)
    check_stats(lib, vm, snap, m, MapOrder(vs - w, w))
    ek, _ = check_evict(lib, vm, ref, m, dev, MapOrder(0, w, False), 4, MapFilter(ANYBITS, vs - 1, 1, 0x7f), host_form=host_form)
    assert len(ek) == 4
    vm.close()
    ref.close()


def run_empty_key(lib, oracle_lib, dev, vs: int, host_form: bool = False) -> None:
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 0, vs, MC.HASH_MAX))
    snap = Snapshot(vm, ref, m, dev)
    order = MapOrder(vs - 8, 8, True)
    assert check_top(lib, vm, snap, m, dev, order, 4, host_form=host_form)[2:] == (0, 0)  # an empty map
    val = (np.arange(vs, dtype=np.uint32) % 251 + 1).astype(np.uint8)[None, :]
    some, d_v = dev(np.zeros(64, dtype=np.uint8)), dev(val)
    settle(d_v)
    fn = lib.map_update_batch_device if on_dev(some) else lib.map_update_batch_staged
    assert fn(vm.h, m, addr(some), addr(d_v), 1, *([None] if on_dev(some) else [])) == 0, lib.last_error(vm.h)
    ref.map_update(m, b"", val.tobytes())
    snap = Snapshot(vm, ref, m, dev)
    for desc in (True, False):
        _, ev, matched, cut = check_top(lib, vm, snap, m, dev, MapOrder(vs - 8, 8, desc), 4, host_form=host_form)
        assert matched == 1 and np.array_equal(ev, val) and cut == int.from_bytes(val[0, vs - 8:].tobytes(), "little")
    check_stats(lib, vm, snap, m, order)
    ek, _ = check_evict(lib, vm, ref, m, dev, order, 1, host_form=host_form)
    assert len(ek) == 1 and ref.map_lookup(m, b"") is None
    snap = Snapshot(vm, ref, m, dev)
    assert check_top(lib, vm, snap, m, dev, order, 4, host_form=host_form)[2:] == (0, 0)
    vm.close()
    ref.close()


def run_vlen0(lib, oracle_lib, dev) -> None:
    """mapscan_cases.run_vlen0's setup: three of a HASH map's four entries are nil-backed and order as
    field 0 whatever bytes their records still hold."""
    from parity import packets
    from test_lru_nil_value import _program
    umem, descs = packets(600, 64, seed=9)
    for d in descs:
        umem[int(d["addr"]) + 1] = 0
    for i in (150, 151, 400):
        umem[int(descs[i]["addr"]) + 1] = 1
    vms = []
    for lb in (lib, oracle_lib):
        vm = VM(Settings(engine=1), lib=lb)
        m = vm.add_map(MapDef(MAP_HASH, 4, 8, 16))
        vm.set_entrypoint(vm.add_raw_program(_program()))
        vms.append((vm, vm.run_batch(umem.copy(), descs)))
    (vm, got), (ref, want) = vms
    assert np.array_equal(got.verdicts, want.verdicts)
    w0 = image_records(vm, m, state_image(vm, m, dev))[0]
    assert int(((w0 & np.uint64(MC.SLOT_VLEN0)) != 0).sum()) == 3, "the batch left no nil-backed records on the device"
    snap = Snapshot(vm, ref, m, dev)
    order = MapOrder(0, 8, False)
    for k in (1, 2, 3, 4):
        _, ev, matched, cut = check_top(lib, vm, snap, m, dev, order, k)
        assert matched == 4 and not ev[:min(k, 3)].any() and (cut == 0) == (k <= 3)
    _, ev, _, cut = check_top(lib, vm, snap, m, dev, MapOrder(0, 8, True), 1)
    assert ev.any() and cut != 0
    st = check_stats(lib, vm, snap, m, order)
    assert st["count"] == 4 and st["min"] == 0 and st["sum"] == st["max"] == cut
    check_evict(lib, vm, ref, m, dev, order, 2)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 6. slot counts
def run_slot_counts(lib, oracle_lib, dev, max_entries: int, slots: int, live: int, host_form: bool = False) -> None:
    rng = np.random.default_rng(slots + 6)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 8, max_entries))
    assert MC.hash_geometry(vm, m)[0] == slots
    keys = SC.keys_for_slots(slots, live)
    vals = rng.integers(0, 256, size=(live, 8), dtype=np.uint8)
    vals[:, 2:] = 0       # 16-bit fields: thousands of entries leave long runs of ties, spread over every tile
    vals[0] = 0xFF        # the first slot's entry ranks first ...
    vals[1] = 0xFF        # ... tied with the last slot's
    vm.map_update_batch_device(m, dev(keys[:2].copy()), dev(vals[:2].copy()))  # first: they get their home slots
    vm.map_update_batch_device(m, dev(keys[2:].copy()), dev(vals[2:].copy()))
    MC.ref_update(ref, m, keys, vals)
    snap = Snapshot(vm, ref, m, dev)
    assert snap.slots[0] == 0 and snap.slots[-1] == slots - 1, "the first and the last slot are to be occupied"
    order = MapOrder(0, 8, True)
    ek, _, _, cut = check_top(lib, vm, snap, m, dev, order, 1, host_form=host_form)
    assert np.array_equal(ek[0], keys[0]) and cut == M64
    ek, _, _, _ = check_top(lib, vm, snap, m, dev, order, 2, host_form=host_form)
    assert np.array_equal(ek, keys[:2])  # the first and the last slot of the table
    for desc in (True, False):
        for k in (live // 2, live - 1, live, live + 9):
            check_top(lib, vm, snap, m, dev, MapOrder(0, 8, desc), k, host_form=host_form)
    check_top(lib, vm, snap, m, dev, MapOrder(0, 8, False), live // 3, MapFilter(ANYBITS, 1, 1, 1), host_form=host_form)
    check_stats(lib, vm, snap, m, order)
    check_stats(lib, vm, snap, m, MapOrder(0, 2), MapFilter(ANYBITS, 1, 1, 1))
    ek, _ = check_evict(lib, vm, ref, m, dev, MapOrder(0, 8, False), live // 2, host_form=host_form)
    assert len(ek) == live // 2
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 7. output discipline
def run_output(lib, oracle_lib, dev, ks: int = 24, vs: int = 100) -> None:
    rng = np.random.default_rng(707)
    n = 130
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 2 * n))
    fill_hash(vm, ref, m, dev, rng, ks, vs, n)
    snap = Snapshot(vm, ref, m, dev)
    live = len(snap.keys)
    order = MapOrder(5, 2, True)
    for koff in ALIGN_OFFSETS:
        for voff in ALIGN_OFFSETS:
            if koff != voff and (koff, voff) not in ((8, 1), (1, 8)):
                continue
            check_top(lib, vm, snap, m, dev, order, 7, koff=koff, voff=voff)
            check_top(lib, vm, snap, m, dev, order, live + 2, MapFilter(ANYBITS, 0, 1, 1), koff=koff, voff=voff)
    for host_form in (False, True):
        check_top(lib, vm, snap, m, dev, order, 9, want_vals=False, host_form=host_form, koff=1)
        check_top(lib, vm, snap, m, dev, order, 9, want_keys=False, host_form=host_form, voff=1)
        check_top(lib, vm, snap, m, dev, order, 9, want_cut=False, host_form=host_form)
        ek, _, matched, cut = check_top(lib, vm, snap, m, dev, order, 0, host_form=host_form, koff=4, voff=4)  # only counts
        assert (len(ek), matched, cut) == (0, live, 0)
        assert raw_top(lib, vm, m, None, order, 0, 0, 11, not host_form) == (0, live, expect_top(snap, None, order, 11)[3])
    check_evict(lib, vm, ref, m, dev, order, 9, koff=1, voff=4)
    check_evict(lib, vm, ref, m, dev, order, 3, want_keys=False, want_vals=False)  # silently
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 8. evict
def run_evict(lib, oracle_lib, dev, host_form: bool = False) -> None:
    rng = np.random.default_rng(88)
    ks, vs = 16, 40
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, MC.HASH_MAX, delete_third=False)  # full
    before = Snapshot(vm, ref, m, dev)
    order = MapOrder(8, 4, False)  # the oldest "last_seen"
    k = 20
    both = expect_top(before, None, order, 2 * k)
    ek, _ = check_evict(lib, vm, ref, m, dev, order, k, host_visit=False, host_form=host_form)
    assert len(ek) == k
    found = to_np(vm.map_lookup_batch(m, dev(keys))[1])
    assert [bool(x) for x in found] == [bytes(key) not in {bytes(e) for e in ek} for key in keys]
    # a second top reports the next k
    snap = Snapshot(vm, ref, m, dev)
    nk, _, matched, _ = check_top(lib, vm, snap, m, dev, order, k, host_form=host_form)
    assert matched == MC.HASH_MAX - k
    want = {bytes(x) for x in both[0]} - {bytes(x) for x in ek}
    assert {bytes(x) for x in nk} == want and len(want) == k
    # the evicted keys learned again take their old records
    nv = rng.integers(0, 256, size=(k, vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(np.ascontiguousarray(ek)), dev(nv))
    MC.ref_update(ref, m, ek, nv)
    img = same_image_map(vm, ref, m, dev, "evicted keys installed again")
    assert int(((image_records(vm, m, img)[0] & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == before.tombs
    after = Snapshot(vm, ref, m, dev)
    assert np.array_equal(after.slots, before.slots), "a key that came back did not take its old record"
    same_map(vm, ref, m, "evicted keys installed again")
    vm.close()
    ref.close()


def run_epoch(lib, dev) -> None:
    vm, m = flow_vm(lib)
    keys, vals = MC.flow_entries(range(8))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    order = MapOrder(0, 8, True)
    vm.epoch_begin()
    k, v, matched, cut, _ = call(lib, vm, m, dev, None, order, 3, 3)
    assert matched == 8 and cut == 6 and sorted(int(x.view(np.uint64)[0]) for x in v[:, :8]) == [6, 7, 8]
    assert raw_stats(lib, vm, m, None, order) == (0, {"count": 8, "sum": 36, "min": 1, "max": 8})
    for device_form in (True, False):
        assert raw_top(lib, vm, m, None, order, 0, 0, 3, device_form, evict=True)[0] == MC.ERR_INVAL
    assert raw_top(lib, vm, m, None, order, 0, 0, 0, True) == (0, 8, 0)
    vm.epoch_end()
    assert raw_top(lib, vm, m, None, order, 0, 0, 3, True, evict=True) == (0, 8, 6)  # silently: no output buffers
    assert vm.map_count(m) == 5
    assert raw_stats(lib, vm, m, None, order) == (0, {"count": 5, "sum": 15, "min": 1, "max": 5})
    vm.close()


# ---------------------------------------------------------------- 9. statistics
def run_stats(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(909)
    ks, vs, n = 8, 24, 300
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 512))
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, n)
    snap = Snapshot(vm, ref, m, dev)
    for width in WIDTHS:
        for off in (0, 3, vs - width):
            check_stats(lib, vm, snap, m, MapOrder(off, width))
            st = check_stats(lib, vm, snap, m, MapOrder(off, width, True), MapFilter(ANYBITS, 20, 1, 3))  # (descending is ignored)
            assert 0 < st["count"] < len(snap.keys)
    assert check_stats(lib, vm, snap, m, MapOrder(0, 8), MapFilter(GT, 0, 1, 0x100))["count"] == 0
    # a sum that wraps 2^64: two entries of all ones
    two = hash_pool(np.random.default_rng(910), ks, 2)
    ones = np.full((2, vs), 0xFF, np.uint8)
    vm.map_update_batch_device(m, dev(two), dev(ones))
    MC.ref_update(ref, m, two, ones)
    snap = Snapshot(vm, ref, m, dev)
    st = check_stats(lib, vm, snap, m, MapOrder(8, 8), MapFilter(EQ, 0, 8, M64))
    assert st == {"count": 2, "sum": M64 - 1, "min": M64, "max": M64}
    assert check_stats(lib, vm, snap, m, MapOrder(8, 8))["max"] == M64
    vm.close()
    ref.close()
    # an ARRAY map: every index counts, the untouched ones as zeros
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 12, 777))
    idx = np.ascontiguousarray(rng.permutation(777)[:400].astype(np.uint32)).view(np.uint8).reshape(-1, 4)
    vals = rng.integers(0, 256, size=(400, 12), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(idx), dev(vals))
    MC.ref_update(ref, m, idx, vals)
    snap = Snapshot(vm, ref, m, dev)
    for width in WIDTHS:
        assert check_stats(lib, vm, snap, m, MapOrder(12 - width, width))["count"] == 777
        check_stats(lib, vm, snap, m, MapOrder(1, width), MapFilter(NE, 0, 4, 0))
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 10. beside traffic
def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    r = Runner(vm, dev, use_async)
    keys, vals = MC.flow_entries(list(range(24)) + [(1 << 41) + i for i in range(8)])
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, rm, keys, vals)

    def ref_run(start: int) -> np.ndarray:
        umem, descs = MC.W.build_batch("c3learn", start, MC.FLOW_PACKETS)
        return ref.run_batch(umem, descs).verdicts

    hits = MapOrder(8, 8, False)  # the hit counter: the eight flows without packets rank first
    v0 = r.run(0)
    w0 = ref_run(0)
    # no xe_sync in between: the evict completes the pipeline itself (compared as a set: an image taken here
    # would complete it first; the order is checked by the top below)
    k, v, matched, cut, _ = call(lib, vm, m, dev, None, hits, 8, 8, evict=True)
    assert np.array_equal(to_np(v0), w0)
    rk, rv = ref.map_dump(rm)
    idle = selects(rv, MapFilter(EQ, 8, 8, 0))
    assert int(idle.sum()) == 8 and matched == len(rk) and cut == 0
    gk, gv = MC.by_key(k, v)
    wk, wv = MC.by_key(rk[idle], rv[idle])
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), "the evicted entries are not the oracle's idle flows"
    MC.ref_delete(ref, rm, rk[idle])
    v1 = r.run(MC.FLOW_PACKETS)
    w1 = ref_run(MC.FLOW_PACKETS)
    snap = Snapshot(vm, ref, m, dev)  # (completes the pipeline; compares the image with the oracle)
    assert np.array_equal(to_np(v1), w1)
    for k in (1, 10, len(snap.keys)):
        check_top(lib, vm, snap, m, dev, MapOrder(8, 8, True), k)   # the top talkers
        check_top(lib, vm, snap, m, dev, hits, k, MapFilter(GE, 8, 8, 2))
    check_stats(lib, vm, snap, m, hits)
    same_map(vm, ref, m, "after two batches and an evict")
    # a host write, then a device top: the map is uploaded first
    nk, _ = MC.flow_entries([1 << 40])
    big = (1 << 60).to_bytes(8, "little") * 2
    vm.map_update(m, nk[0].tobytes(), big)
    ref.map_update(rm, nk[0].tobytes(), big)
    up, _ = vm.map_traffic(m)
    assert raw_top(lib, vm, m, None, MapOrder(8, 8, True), 0, 0, 1, True) == (0, len(snap.keys) + 1, 1 << 60)
    assert vm.map_traffic(m)[0] == up + 1
    v2 = r.run(2 * MC.FLOW_PACKETS)
    w2 = ref_run(2 * MC.FLOW_PACKETS)
    same_map(vm, ref, m, "after three batches")
    assert np.array_equal(to_np(v2), w2)
    vm.close()
    ref.close()


def run_traffic(lib, dev) -> None:
    vm, m = flow_vm(lib)
    r = Runner(vm, dev, False)
    keys, vals = MC.flow_entries(list(range(56)) + [(1 << 41) + i for i in range(8)])  # eight flows without packets
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    r.run(0)  # the map is now newer on the device
    up, down = vm.map_traffic(m)
    hits = MapOrder(8, 8, False)
    for flt in (None, MapFilter(EQ, 8, 8, 0), MapFilter(NE, 8, 8, 0)):
        k, v, matched, cut, _ = call(lib, vm, m, dev, flt, MapOrder(8, 8, True), 10, 10)
        assert matched >= 8 and raw_stats(lib, vm, m, flt, hits)[1]["count"] == matched
    k, v, matched, cut, _ = call(lib, vm, m, dev, None, hits, 5, 8, evict=True)
    assert matched >= 64 and len(k) == 5 and cut == 0 and not v[:, 8:].any()  # (five of the eight never hit)
    # the delta base went to zero with the values: xe_map_delta reports nothing on the evicted records
    out = dev(np.full(vm.map_values_bytes(m), GUARD, np.uint8))
    settle(out)
    vm.map_delta(m, addr(out), lane=8)
    delta = to_np(out).reshape(-1, 16)
    w0, ikeys, _, _ = image_records(vm, m, state_image(vm, m, dev))
    for key in k:
        slot = np.nonzero((ikeys == key).all(axis=1) & (w0 == np.uint64(MC.SLOT_TOMB)))[0]
        assert len(slot) == 1 and key.any() and not delta[slot[0]].any(), "an evict left the delta base behind"
    assert delta.any(), "the batch's adds are not in the delta"
    assert vm.map_traffic(m) == (up, down), "a top, an evict or a stats call moved the whole map"
    r.run(MC.FLOW_PACKETS)  # a batch after the device evict: nothing to upload
    assert vm.map_traffic(m) == (up, down)
    vm.close()


# ---------------------------------------------------------------- 11. limits
def run_limits(lib, oracle_lib, dev) -> None:
    good = N.MapOrder(0, 8, 1, 0)
    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        d = MapDef(t, 4, 8, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 8, 16)
        m = vm.add_map(d)
        k, v = np.zeros((2, 4), np.uint8), np.zeros((2, 8), np.uint8)
        for device_form in (True, False):
            for evict in (False, True):
                assert raw_top(lib, vm, m, None, good, k.ctypes.data, v.ctypes.data, 2, device_form, evict)[0] == MC.ERR_UNSUPPORTED
                assert b"ARRAY and HASH" in lib.last_error(vm.h)
        assert raw_stats(lib, vm, m, None, good)[0] == MC.ERR_UNSUPPORTED
        vm.close()

    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 8, 10))
    for device_form in (True, False):
        assert raw_top(lib, vm, m, None, good, 0, 0, 2, device_form, evict=True)[0] == MC.ERR_INVAL  # as xe_map_delete
    assert raw_top(lib, vm, m, None, good, 0, 0, 2, True) == (0, 10, 0)
    vm.close()
    ref.close()

    rng = np.random.default_rng(1111)
    vs = 13
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, vs, MC.HASH_MAX))
    fill_hash(vm, ref, m, dev, rng, 8, vs, 30)
    before = state_image(vm, m, dev)
    bad_orders = [None,                                                                   # ord NULL
                  N.MapOrder(0, 0, 0, 0), N.MapOrder(0, 3, 0, 0), N.MapOrder(0, 16, 1, 0),  # width
                  N.MapOrder(0, 8, 0, 1), N.MapOrder(0, 8, 1, 0xffffffff),                 # pad
                  N.MapOrder(0, 8, 2, 0), N.MapOrder(0, 1, 0xffffffff, 0),                 # descending
                  N.MapOrder(vs, 1, 0, 0), N.MapOrder(vs - 7, 8, 1, 0), N.MapOrder(0xffffffff, 8, 0, 0),
                  N.MapOrder(0xfffffffc, 4, 0, 0)]                                         # a field outside the value
    for o in bad_orders:
        what = None if o is None else (o.offset, o.width, o.descending, o.pad)
        for device_form in (True, False):
            for evict in (False, True):
                assert raw_top(lib, vm, m, None, o, 0, 0, 5, device_form, evict)[0] == MC.ERR_INVAL, what
        if o is None or o.descending <= 1:  # (stats ignores descending)
            assert raw_stats(lib, vm, m, None, o)[0] == MC.ERR_INVAL, what
    ok = N.MapOrder(vs - 8, 8, 1, 0)
    bad_filters = [N.MapFilter(9, 0, 1, 0, 0), N.MapFilter(EQ, 0, 1, 1, 0), N.MapFilter(EQ, 0, 3, 0, 0), N.MapFilter(EQ, vs, 1, 0, 0),
                   N.MapFilter(EQ, vs - 7, 8, 0, 0), N.MapFilter(EQ, 0xfffffffc, 4, 0, 0)]
    for f in bad_filters:
        for device_form in (True, False):
            for evict in (False, True):
                assert raw_top(lib, vm, m, f, ok, 0, 0, 5, device_form, evict)[0] == MC.ERR_INVAL, (f.op, f.offset, f.width, f.pad)
        assert raw_stats(lib, vm, m, f, ok)[0] == MC.ERR_INVAL
    for device_form in (True, False):
        for evict in (False, True):
            assert raw_top(lib, vm, m, None, ok, 0, 0, 5, device_form, evict, matched=False)[0] == MC.ERR_INVAL  # a NULL matched
            assert raw_top(lib, vm, 99, None, ok, 0, 0, 5, device_form, evict)[0] == MC.ERR_INVAL  # a bad map index
    assert raw_stats(lib, vm, m, None, ok, out=False)[0] == MC.ERR_INVAL
    assert raw_stats(lib, vm, 99, None, ok)[0] == MC.ERR_INVAL
    assert raw_top(lib, vm, m, None, ok, 0, 0, 1 << 40, True)[:2] == (0, 20)  # a k past any table
    assert np.array_equal(before, state_image(vm, m, dev)), "a refused call changed the map"
    same_map(vm, ref, m, "after the refused calls")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 12. determinism
def run_determinism(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(1212)
    ks, vs, n = 24, 65, 3000
    mdef = MapDef(MAP_HASH, ks, vs, 4096)
    vm, ref, m, _ = pair(lib, oracle_lib, mdef)
    keys = hash_pool(rng, ks, n)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    vals[:, 4:] = 0  # a 16-bit order field at +3 .. +4 with one byte zero: runs of ties
    gone = np.ascontiguousarray(keys[::3])

    def build(v: VM, mi: int) -> None:
        # through the host mirror, key by key: a device batch places colliding keys in the order its lanes
        # win their claims, so two such builds hold the same entries in tables that may differ
        v.map_update_batch(mi, keys, vals)
        assert to_np(v.map_delete_batch(mi, dev(gone))).all()

    build(vm, m)
    MC.ref_update(ref, m, keys, vals)
    MC.ref_delete(ref, m, gone)
    order, flt, k = MapOrder(3, 2, True), MapFilter(ANYBITS, 0, 1, 7), 777
    first = call(lib, vm, m, dev, flt, order, k, k, koff=4, voff=1)
    second = call(lib, vm, m, dev, flt, order, k, k, koff=4, voff=1)
    assert first[2:4] == second[2:4] and first[2] > k
    assert np.array_equal(first[4][0], second[4][0]) and np.array_equal(first[4][1], second[4][1])
    snap = Snapshot(vm, ref, m, dev)
    ek, ev, matched, cut, _ = expect_top(snap, flt, order, k)
    assert np.array_equal(first[0], ek) and np.array_equal(first[1], ev) and first[2:4] == (matched, cut)
    # the same state rebuilt in a fresh VM, exported and imported into a third
    vm2 = VM(Settings(engine=1), lib=lib)
    m2 = vm2.add_map(mdef)
    build(vm2, m2)
    img = dev(np.zeros(vm2.map_state_bytes(m2), dtype=np.uint8))
    settle(img)
    vm2.map_state_export(m2, addr(img))
    vm3 = VM(Settings(engine=1), lib=lib)
    m3 = vm3.add_map(mdef)
    vm3.map_state_import(m3, addr(img))
    for v, mi in ((vm2, m2), (vm3, m3)):
        again = call(lib, v, mi, dev, flt, order, k, k, koff=4, voff=1)
        assert again[2:4] == first[2:4]
        assert np.array_equal(again[4][0], first[4][0]) and np.array_equal(again[4][1], first[4][1])
        v.close()
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 13. the Python interface
def run_python_api(lib, oracle_lib, dev, on_device: bool) -> None:
    rng = np.random.default_rng(1313)
    ks, vs = 8, 24
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, 40, delete_third=False)
    vals[:, 9:] = 0
    vals[:, 8] &= 7  # an 8-byte field at +8 with eight values: ties
    vals[0, 8:16] = 0xFF  # ... and one with bit 63 set
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, m, keys, vals)
    snap = Snapshot(vm, ref, m, dev)
    flt = MapFilter(ANYBITS, 2, 1, 0x3f)
    for desc in (True, False):
        order = MapOrder(8, 8, desc)
        ek, ev, matched, cut, _ = expect_top(snap, flt, order, 12)
        k, v, gm, gc = vm.map_top(m, order, 12, flt, on_device=on_device, ranked=False)
        assert on_dev(k) == on_device and (gm, gc) == (matched, cut)
        assert np.array_equal(to_np(k), ek) and np.array_equal(to_np(v), ev)
        # ranked: by the field in the direction, ties in the reported (slot) order
        f = [int(x) for x in fields(ev, 8, 8)]
        rank = sorted(range(len(f)), key=lambda i: (-f[i] if desc else f[i], i))
        k, v, gm, gc = vm.map_top(m, order, 12, flt, on_device=on_device)
        assert on_dev(k) == on_device and (gm, gc) == (matched, cut)
        assert np.array_equal(to_np(k), ek[rank]) and np.array_equal(to_np(v), ev[rank])
    k, v, gm, gc = vm.map_top(m, MapOrder(8, 8), 1 << 40, on_device=on_device, ranked=False)  # a k past the table
    assert gm == 40 and np.array_equal(to_np(k), snap.keys) and gc == 0
    assert vm.map_stats(m, MapOrder(8, 8), flt) == expect_stats(snap, flt, MapOrder(8, 8))
    assert vm.map_stats(m, MapOrder(8, 8))["max"] == M64
    order = MapOrder(8, 8, False)
    ek, ev, matched, cut, _ = expect_top(snap, flt, order, 6)
    k, v, gm, gc = vm.map_evict(m, order, 6, flt, on_device=on_device, ranked=False)
    assert (gm, gc) == (matched, cut) and np.array_equal(to_np(k), ek) and np.array_equal(to_np(v), ev)
    MC.ref_delete(ref, m, ek)
    same_image_map(vm, ref, m, dev, "after map_evict")
    same_map(vm, ref, m, "after map_evict")
    assert vm.map_stats(m, MapOrder(8, 8), flt)["count"] == matched - 6
    # an ARRAY map: u32 indices
    am = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 10))
    vm.map_update(am, (7).to_bytes(4, "little"), b"\x05" * 8)
    vm.map_update(am, (2).to_bytes(4, "little"), b"\x05" * 8)
    k, v, gm, gc = vm.map_top(am, MapOrder(0, 4), 3, on_device=on_device)
    assert gm == 10 and gc == 0 and to_np(k).view(np.uint32).reshape(-1).tolist() == [2, 7, 0]
    vm.close()
    ref.close()
