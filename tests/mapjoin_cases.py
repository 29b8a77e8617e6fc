"""Shared cases of the device-side join (xe_map_join_device / xe_map_join): tests/test_mapjoin.py runs them on the
host simulation, tests/test_mapjoin_gpu.py on the product library.

No expected value comes from the code under test:
  * the candidates are the source's mapscan_cases.Snapshot (the oracle's entries, in the slot order of the
    exported image) filtered by mapscan_cases.selects;
  * "present" is a Python lookup of the join bytes in the oracle's dump of the other map (Other), pinned by the
    hand-worked JOIN_TABLE; the other map's values come from the same dump;
  * after a removal the oracle deletes the same keys one by one and the maps are compared as the scan's expire
    cases compare them (the image, the plain tombstones that kept their key words, the count);
  * the other map's exported image must not change at all, nor the source's when nothing is removed.

Sizes (xe_mapops.h / xe_mapops.hip): a tile is 256 slots in 4 rounds of 64 lanes; the tile launcher gives every
tile a wave of its own up to 256 workgroups of 4 waves, then a quarter of that, so the 2,048 tiles of a 2^19-slot
source are strided over by 1,024 waves; the other map's records have 2 words (keys up to 8 bytes: find_grouped<2>),
4 words (up to 24: find_grouped<4>) or more (mo_find); JOIN_VALUE's sub-groups follow the other map's value size
(1, 4, 16 or 64 lanes, cut at 16, 64 and 1,024 bytes)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import mapops_cases as MC
import mapscan_cases as SC
from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, MG_KEY, MG_VALUE,
                                  MJ_ABSENT, MJ_PRESENT, MJ_REMOVE, VM, MapDef, MapFilter, MapJoin, Settings)
from mapgroup_cases import EDGE_COUNTS, KEY_SHAPES, array_rows, install, remove, two_maps, u64_rows
from mapops_cases import (GUARD, addr, flow_vm, guards_intact, hash_pool, home_slot, image_records, keys_with_home, on_dev, place,
                          same_image_map, same_map, settle, state_image, to_np, Runner)
from mapscan_cases import ANYBITS, EQ, GT, NE, Snapshot, fields, selects

MODES = (MJ_PRESENT, MJ_ABSENT)
# the group's shapes and an 8-byte one: other records of 2 words (3, 4, 8 key bytes), 4 words (13, 24) and 16 (64)
JOIN_SHAPES = KEY_SHAPES + ((MG_VALUE, 2, 8),)
OTHER_VALUE_SIZES = (8, 24, 100, 1100)  # JOIN_VALUE with 1, 4, 16 and 64 lanes an entry
SHAPE_SRC_VS = 72
CHAIN_KEY_SIZES = (8, 13, 64)


# ---------------------------------------------------------------- the join, restated
class Other:
    """The oracle's entries of the other map: lookup(join bytes) -> its value row, or None when absent."""

    def __init__(self, ref: VM, m: int):
        d = ref.map_defs[m]
        self.array, self.vs = d.type == MAP_ARRAY, d.value_size
        if self.array:
            self.rows = np.frombuffer(ref.map_dump(m), dtype=np.uint8).reshape(d.max_entries, d.value_size)
        else:
            k, v = ref.map_dump(m)
            self.rows = {bytes(kk.tobytes()): vv for kk, vv in zip(k, v)}

    def lookup(self, jb: bytes):
        if self.array:
            i = int.from_bytes(jb, "little")
            return self.rows[i] if i < len(self.rows) else None
        return self.rows.get(jb)


def expect_rows(keys: np.ndarray, vals: np.ndarray, j: MapJoin, lookup, ovs: int):
    """(kept mask, the other map's value row for every entry: zeros where absent) over candidate rows."""
    src = keys if j.from_ == MG_KEY else vals
    kept = np.zeros(len(src), dtype=bool)
    ovals = np.zeros((len(src), ovs), dtype=np.uint8)
    for i in range(len(src)):
        hit = lookup(src[i, j.offset:j.offset + j.len].tobytes())
        kept[i] = (hit is not None) == (j.mode == MJ_PRESENT)
        if hit is not None and j.mode == MJ_PRESENT:
            ovals[i] = hit
    return kept, ovals


def _rows(*rows):
    return np.array(rows, dtype=np.uint8)


# (keys, values, spec, the other map as a dict, kept, other values), worked out by hand
JOIN_TABLE = (
    # by key bytes 1..2: the first and the third entry's are in the other map
    (_rows((9, 1, 2, 7), (8, 1, 3, 6), (9, 1, 2, 0)), _rows((5,), (6,), (7,)), MapJoin(MG_KEY, 1, 2, MJ_PRESENT),
     {b"\x01\x02": _rows((0xaa, 0xbb))[0]}, [True, False, True], _rows((0xaa, 0xbb), (0, 0), (0xaa, 0xbb))),
    # the same, absent: the second alone, and the other values are zeros
    (_rows((9, 1, 2, 7), (8, 1, 3, 6), (9, 1, 2, 0)), _rows((5,), (6,), (7,)), MapJoin(MG_KEY, 1, 2, MJ_ABSENT),
     {b"\x01\x02": _rows((0xaa, 0xbb))[0]}, [False, True, False], _rows((0, 0), (0, 0), (0, 0))),
    # by value byte 0
    (_rows((1,), (2,)), _rows((5, 1), (6, 1)), MapJoin(MG_VALUE, 0, 1, MJ_PRESENT), {b"\x06": _rows((3,))[0]},
     [False, True], _rows((0,), (3,))),
)


def check_join_table() -> None:
    for keys, vals, j, other, kept, ovals in JOIN_TABLE:
        got = expect_rows(keys, vals, j, other.get, ovals.shape[1])
        assert got[0].tolist() == kept and np.array_equal(got[1], ovals), (j, got)


# ---------------------------------------------------------------- the call and its check
def c_filter(flt):
    return None if flt is None else (flt if isinstance(flt, N.MapFilter) else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand))


def c_join(j, flags: int = 0):
    if j is None or isinstance(j, N.MapJoin):
        return j
    return N.MapJoin(j.from_, j.offset, j.len, j.mode, flags, 0)


def raw_join(lib, vm: VM, src: int, flt, j, other: int, kptr=0, vptr=0, optr=0, cap: int = 0, flags: int = 0, device_form: bool = True,
             matched: bool = True, selected: bool = True):
    """One call by address. Returns (rc, matched, selected)."""
    cf, cj = c_filter(flt), c_join(j, flags)
    n, sel = C.c_uint64(0xDEADBEEF), C.c_uint64(0xDEADBEEF)
    head = (vm.h, src, None if cf is None else C.byref(cf), None if cj is None else C.byref(cj), other, kptr or None, vptr or None,
            optr or None, cap, C.byref(n) if matched else None, C.byref(sel) if selected else None)
    rc = lib.map_join_device(*head, None) if device_form else lib.map_join(*head)
    return rc, n.value, sel.value


def expect_join(snap: Snapshot, ref: VM, other: int, j: MapJoin, flt):
    """(keys, values, other values) of the kept entries in the order the call reports them, and the candidates' number."""
    oth = Other(ref, other)
    snap.expect(flt)  # the candidate set is the oracle's
    cand = selects(snap.vals, flt)
    k, v = snap.keys[cand], snap.vals[cand]
    kept, ovals = expect_rows(k, v, j, oth.lookup, oth.vs)
    return k[kept], v[kept], ovals[kept], int(cand.sum())


def check_join(lib, vm: VM, ref: VM, src: int, other: int, dev, j: MapJoin, flt=None, cap=None, rm: bool = False,
               outs=(True, True, True), host_form: bool = False, snap: Snapshot | None = None, what: str = ""):
    """A join against the snapshot of the source and the oracle's other map: the totals, the first r rows of the
    three outputs, the guard bytes behind entry r; the other map's image unchanged, the source's unchanged or, after
    a removal, equal to the oracle's after deleting the same keys. Returns (expected keys, r, matched, selected)."""
    snap = snap or Snapshot(vm, ref, src, dev)
    ek, ev, eo, ncand = expect_join(snap, ref, other, j, flt)
    cap = len(ek) if cap is None else cap
    r = min(cap, len(ek))
    d, od = vm.map_defs[src], vm.map_defs[other]
    ks = 4 if d.type == MAP_ARRAY else d.key_size
    mk = np.ascontiguousarray if host_form else dev
    room = r + 3
    bufs = [place(mk, np.full((room, w), GUARD, np.uint8), 0)[0] for w in (ks, d.value_size, od.value_size)]
    for b in bufs:
        settle(b)
    before = state_image(vm, src, dev), state_image(vm, other, dev)
    ptrs = [addr(b) if want else 0 for b, want in zip(bufs, outs)]
    rc, matched, selected = raw_join(lib, vm, src, flt, j, other, *ptrs, cap=cap, flags=MJ_REMOVE if rm else 0, device_form=not host_form)
    what = what or f"join {j} filter {flt} cap {cap} remove {rm} outputs {outs}"
    assert rc == 0, f"{what}: {lib.last_error(vm.h)}"
    assert matched == len(ek), f"{what}: matched {matched}, expected {len(ek)}"
    assert selected == ncand, f"{what}: selected {selected}, expected {ncand}"
    for b, want, w, exp, name in zip(bufs, outs, (ks, d.value_size, od.value_size), (ek, ev, eo), ("keys", "values", "other values")):
        got = guards_intact(b, 0, r * w if want else 0, f"{what}: {name}")
        if want:
            assert np.array_equal(got.reshape(r, w), exp[:r]), f"{what}: {name} differ (or their order)"
    if other != src or not rm:
        assert np.array_equal(before[1], state_image(vm, other, dev)), f"{what}: the other map changed"
    if not rm:
        assert np.array_equal(before[0], state_image(vm, src, dev)), f"{what}: the source changed"
        return ek, r, matched, selected
    MC.ref_delete(ref, src, ek[:r])
    img = same_image_map(vm, ref, src, dev, what)
    w0, keys, vals, count = image_records(vm, src, img)
    byk = {bytes(k.tobytes()): s for k, s in zip(snap.keys, snap.slots)}
    gone = np.array([byk[bytes(k.tobytes())] for k in ek[:r]], dtype=np.int64)
    assert (w0[gone] == np.uint64(MC.SLOT_TOMB)).all(), f"{what}: a removed record is not a plain tombstone"
    assert np.array_equal(keys[gone], ek[:r]), f"{what}: a removed record lost its key words"
    assert not vals[gone].any(), f"{what}: a removed record's value is not zero"
    assert count == len(snap.keys) - r
    assert int(((w0 & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == snap.tombs + r
    return ek, r, matched, selected


def fill(vm, ref, m, dev, keys, vals):
    install(vm, ref, m, dev, np.ascontiguousarray(keys), np.ascontiguousarray(vals))


# ---------------------------------------------------------------- 1. tile and round edges
def run_edges(lib, oracle_lib, dev, live: int, mode: int) -> None:
    """`live` source entries among the tombstones of half as many deleted ones; every second one's key is in the
    other map. cap_entries below, at and above matched, guard bytes behind entry r of all three outputs."""
    rng = np.random.default_rng(2000 + live)
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, 512), MapDef(MAP_HASH, 8, 24, 512))
    extra = (live + 1) // 2
    keys = hash_pool(rng, 8, live + extra + 20)
    vals = rng.integers(0, 256, size=(len(keys), 16), dtype=np.uint8)
    fill(vm, ref, src, dev, keys[:live + extra], vals[:live + extra])
    remove(vm, ref, src, dev, keys[live:live + extra])
    okeys = np.concatenate([keys[0:live:2], keys[live:live + extra:3], keys[live + extra:]])  # present, deleted in src, unrelated
    fill(vm, ref, other, dev, okeys, rng.integers(1, 256, size=(len(okeys), 24), dtype=np.uint8))
    snap = Snapshot(vm, ref, src, dev)
    assert len(snap.keys) == live and snap.tombs == extra
    j = MapJoin(MG_KEY, 0, 8, mode)
    want = (live + 1) // 2 if mode == MJ_PRESENT else live // 2
    for cap in sorted({max(want - 1, 0), want, want + 5}):
        _, r, matched, selected = check_join(lib, vm, ref, src, other, dev, j, cap=cap, snap=snap)
        assert (matched, selected, r) == (want, live, min(cap, want))
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. striding waves
def run_striding(lib, oracle_lib, dev) -> None:
    """mapgroup_cases.run_striding's source: 2^19 slots, about half full, 2,048 tiles for 1,024 waves; the other map
    holds 750 of the 1,500 values of a 2-byte field. (The oracle is not given 250,000 entries one by one: the
    candidates are the installed arrays, tied to the map by the exported image.)"""
    slots, n = 1 << 19, 250_000
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 8, slots // 2), MapDef(MAP_HASH, 2, 16, 2048))
    assert MC.hash_geometry(vm, src)[0] == slots
    c = np.arange(1, n + 1, dtype=np.uint64)
    keys = u64_rows(c)
    vals = u64_rows(((c * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(1500) + (c << np.uint64(16)))
    vm.map_update_batch_device(src, dev(keys), dev(vals))
    okeys = np.arange(0, 1500, 2, dtype=np.uint16).view(np.uint8).reshape(-1, 2).copy()
    ovals = np.random.default_rng(5).integers(1, 256, size=(750, 16), dtype=np.uint8)
    fill(vm, ref, other, dev, okeys, ovals)
    img = state_image(vm, src, dev)
    w0, ikeys, ivals, count = image_records(vm, src, img)
    full = np.nonzero(w0 & np.uint64(MC.SLOT_FULL))[0]
    assert count == len(full) == n
    sk, sv = ikeys[full], ivals[full]
    order = np.argsort(sk.view(np.uint64).reshape(-1))
    assert np.array_equal(sk[order], keys) and np.array_equal(sv[order], vals), "the image's entries are not the installed ones"
    field = fields(sv, 0, 2)
    even = (field % np.uint64(2)) == 0
    oimg = state_image(vm, other, dev)
    j = MapJoin(MG_VALUE, 0, 2, MJ_PRESENT)
    room = 1000
    bufs = [dev(np.full((room + 2, w), GUARD, np.uint8)) for w in (8, 8, 16)]
    for b in bufs:
        settle(b)
    rc, matched, selected = raw_join(lib, vm, src, None, j, other, *[addr(b) for b in bufs], cap=room)
    assert (rc, matched, selected) == (0, int(even.sum()), n), lib.last_error(vm.h)
    gk, gv, go = (to_np(b) for b in bufs)
    assert np.array_equal(gk[:room], sk[even][:room]) and np.array_equal(gv[:room], sv[even][:room])
    assert np.array_equal(go[:room], ovals[(field[even][:room] // np.uint64(2)).astype(np.int64)])
    assert all((to_np(b)[room:] == GUARD).all() for b in bufs), "bytes behind entry r were written"
    assert raw_join(lib, vm, src, None, MapJoin(MG_VALUE, 0, 2, MJ_ABSENT), other) == (0, n - int(even.sum()), n)
    assert np.array_equal(img, state_image(vm, src, dev)) and np.array_equal(oimg, state_image(vm, other, dev)), "a map changed"
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. every probe path of the other map
def run_shape(lib, oracle_lib, dev, shape) -> None:
    """One join shape (from, offset, len) against other maps of that key size, one per value sub-group width: half
    of the join values present, all of them, none (an empty map); both modes; the empty candidate set."""
    frm, off, ln = shape
    rng = np.random.default_rng(8000 + 100 * off + ln + frm)
    n = 40
    vm, ref, src, _ = MC.pair(lib, oracle_lib, MapDef(MAP_HASH, 64, SHAPE_SRC_VS, 64))
    keys = hash_pool(rng, 64, n)
    vals = rng.integers(0, 256, size=(n, SHAPE_SRC_VS), dtype=np.uint8)
    rep = rng.integers(0, 12, size=n)  # about a dozen join values
    if frm == MG_KEY:
        keys[:, off:off + ln] = keys[rep, off:off + ln]
        keys = np.unique(keys, axis=0)
        vals = vals[:len(keys)]
    else:
        vals[:, off:off + ln] = vals[rep, off:off + ln]
    fill(vm, ref, src, dev, keys, vals)
    snap = Snapshot(vm, ref, src, dev)
    jvals = np.unique((keys if frm == MG_KEY else vals)[:, off:off + ln], axis=0)
    assert 2 <= len(jvals) <= 12
    others = {}
    for ovs in OTHER_VALUE_SIZES:
        m = vm.add_map(MapDef(MAP_HASH, ln, ovs, 64))
        assert ref.add_map(MapDef(MAP_HASH, ln, ovs, 64)) == m
        others[ovs] = m
    empty = vm.add_map(MapDef(MAP_HASH, ln, 8, 64))
    ref.add_map(MapDef(MAP_HASH, ln, 8, 64))
    stray = hash_pool(rng, ln, 20) if ln > 1 else np.zeros((0, 1), np.uint8)
    for ovs, m in others.items():
        present = jvals if ovs == 24 else jvals[::2]  # the 24-byte one holds every join value
        ok = np.unique(np.concatenate([present, stray]), axis=0)
        fill(vm, ref, m, dev, ok, rng.integers(1, 256, size=(len(ok), ovs), dtype=np.uint8))
    for mode in MODES:
        j = MapJoin(frm, off, ln, mode)
        for ovs, m in others.items():
            _, _, matched, selected = check_join(lib, vm, ref, src, m, dev, j, snap=snap)
            assert selected == len(snap.keys)
            if ovs == 24:
                assert matched == (selected if mode == MJ_PRESENT else 0)  # all present
            else:
                assert 0 < matched < selected
        _, _, matched, _ = check_join(lib, vm, ref, src, empty, dev, j, snap=snap)  # none present
        assert matched == (0 if mode == MJ_PRESENT else len(snap.keys))
        # the empty candidate set (no byte of a 72-byte random value is above 255)
        _, _, matched, selected = check_join(lib, vm, ref, src, others[8], dev, j, MapFilter(GT, 0, 1, 0xfff), snap=snap)
        assert (matched, selected) == (0, 0)
    # keys alone, values alone, other values alone; the host-pointer form
    j = MapJoin(frm, off, ln, MJ_PRESENT)
    for outs in ((True, False, False), (False, True, False), (False, False, True)):
        check_join(lib, vm, ref, src, others[100], dev, j, cap=3, outs=outs, snap=snap)
    check_join(lib, vm, ref, src, others[1100], dev, j, snap=snap, host_form=True)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 4. chains in the other map
def run_chains(lib, oracle_lib, dev, ks: int) -> None:
    """An other map of 16 slots; nine keys that all have their home in slot 14. Eight are installed one after
    another: the chain occupies slots 14, 15, 0 .. 5 and wraps the table's end. The second and the fourth are
    deleted again: tombstones that keep their key words stand in the chain. The later keys are present through
    the tombstones, the deleted ones absent, and so is the ninth, whose probe runs the whole chain to a free slot."""
    want = {s for s in range(MC.HASH_CAP) if s & 15 == 14}
    gkeys = keys_with_home(ks, want, 9)
    assert all(home_slot(k, 16) == 14 for k in gkeys)
    svs = ks + 7
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, svs, 256), MapDef(MAP_HASH, ks, 20, 8))
    assert MC.hash_geometry(vm, other)[0] == 16
    rng = np.random.default_rng(99 + ks)
    ok = np.array([np.frombuffer(k, np.uint8) for k in gkeys])
    for i in range(8):  # one by one: the chain's order is the insertion order
        fill(vm, ref, other, dev, ok[i:i + 1], rng.integers(1, 256, size=(1, 20), dtype=np.uint8))
    remove(vm, ref, other, dev, ok[[1, 3]])
    w0 = image_records(vm, other, state_image(vm, other, dev))[0]
    assert set(np.nonzero(w0[:16] & np.uint64(MC.SLOT_FULL))[0].tolist()) == {14, 0, 2, 3, 4, 5}, "the chain did not wrap"
    assert set(np.nonzero(w0[:16] & np.uint64(MC.SLOT_TOMB))[0].tolist()) == {15, 1}
    n = 90
    keys = hash_pool(rng, 8, n)
    vals = rng.integers(0, 256, size=(n, svs), dtype=np.uint8)
    which = np.arange(n) % 9
    vals[:, 5:5 + ks] = ok[which]
    fill(vm, ref, src, dev, keys, vals)
    for mode in MODES:
        _, _, matched, selected = check_join(lib, vm, ref, src, other, dev, MapJoin(MG_VALUE, 5, ks, mode))
        assert (matched, selected) == ((60 if mode == MJ_PRESENT else 30), n)  # six of nine keys are present
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 5. nil-backed values
def run_vlen0(lib, oracle_lib, dev) -> None:
    """mapgroup_cases.run_vlen0's setup: three of the four entries (keys 0 .. 3) of a HASH map are nil-backed. As a
    source their join bytes read as zeros; as the other map they are present and their values are reported as zeros."""
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
        by_val = vm.add_map(MapDef(MAP_HASH, 2, 16, 8))
        feed = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 6))
        vm.set_entrypoint(vm.add_raw_program(_program()))
        vms.append((vm, vm.run_batch(umem.copy(), descs)))
    (vm, got), (ref, want) = vms
    assert np.array_equal(got.verdicts, want.verdicts)
    w0 = image_records(vm, m, state_image(vm, m, dev))[0]
    assert int(((w0 & np.uint64(MC.SLOT_VLEN0)) != 0).sum()) == 3, "the batch left no nil-backed records on the device"
    snap = Snapshot(vm, ref, m, dev)
    assert int((~snap.vals.any(axis=1)).sum()) == 3
    # a source: the three nil-backed entries' value bytes 0 .. 1 read as 0 0, which the other map holds
    fill(vm, ref, by_val, dev, _rows((0, 0), (9, 9)), np.full((2, 16), 7, np.uint8))
    _, _, matched, _ = check_join(lib, vm, ref, m, by_val, dev, MapJoin(MG_VALUE, 0, 2, MJ_PRESENT), snap=snap)
    assert matched == 3
    _, _, matched, _ = check_join(lib, vm, ref, m, by_val, dev, MapJoin(MG_VALUE, 0, 2, MJ_ABSENT), snap=snap)
    assert matched == 1
    # the other map: indices 0 .. 5 of an ARRAY against keys 0 .. 3; present, nil-backed or not, values as zeros
    fill(vm, ref, feed, dev, array_rows(6), np.full((6, 8), 3, np.uint8))
    ek, r, matched, _ = check_join(lib, vm, ref, feed, m, dev, MapJoin(MG_KEY, 0, 4, MJ_PRESENT))
    assert matched == 4 and ek.view(np.uint32).reshape(-1).tolist() == [0, 1, 2, 3]
    _, _, eo, _ = expect_join(Snapshot(vm, ref, feed, dev), ref, m, MapJoin(MG_KEY, 0, 4, MJ_PRESENT), None)
    assert int((~eo.any(axis=1)).sum()) == 3 and eo.any(), "the oracle does not report the nil-backed values as zeros"
    ek, _, matched, _ = check_join(lib, vm, ref, feed, m, dev, MapJoin(MG_KEY, 0, 4, MJ_ABSENT))
    assert matched == 2 and ek.view(np.uint32).reshape(-1).tolist() == [4, 5]
    # a self-join of the nil-backed map by its own key
    _, _, matched, _ = check_join(lib, vm, ref, m, m, dev, MapJoin(MG_KEY, 0, 4, MJ_PRESENT), snap=snap)
    assert matched == 4
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 6. ARRAY on either side
def run_array_sides(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(606)
    # an ARRAY source's index bytes as the join key, against HASH maps and against ARRAYs
    vm, ref, src, h1 = two_maps(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 12, 777), MapDef(MAP_HASH, 1, 16, 256))
    vals = rng.integers(0, 256, size=(777, 12), dtype=np.uint8)
    fill(vm, ref, src, dev, array_rows(777), vals)
    snap = Snapshot(vm, ref, src, dev)
    fill(vm, ref, h1, dev, _rows((0,), (1,), (2,), (200,)), rng.integers(1, 256, size=(4, 16), dtype=np.uint8))
    _, _, matched, _ = check_join(lib, vm, ref, src, h1, dev, MapJoin(MG_KEY, 0, 1, MJ_PRESENT), snap=snap)
    assert matched == 4 + 4 + 4 + 3  # indices whose low byte is 0, 1, 2 (0, 256, 512, 768 ...) or 200 (200, 456, 712)
    _, _, matched, _ = check_join(lib, vm, ref, src, h1, dev, MapJoin(MG_KEY, 1, 1, MJ_ABSENT), snap=snap)
    assert matched == 9  # the second index byte is 0, 1 or 2 for all but indices 768 .. 776, where it is 3
    h4 = vm.add_map(MapDef(MAP_HASH, 4, 8, 64))
    ref.add_map(MapDef(MAP_HASH, 4, 8, 64))
    some = np.array([5, 255, 256, 776, 777, 70000], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    fill(vm, ref, h4, dev, some, rng.integers(1, 256, size=(6, 8), dtype=np.uint8))
    ek, _, matched, _ = check_join(lib, vm, ref, src, h4, dev, MapJoin(MG_KEY, 0, 4, MJ_PRESENT), snap=snap)
    assert ek.view(np.uint32).reshape(-1).tolist() == [5, 255, 256, 776]
    # ARRAY others: len 1, 2 and 4; an index at and beyond max_entries is absent
    for off, ln, entries, present in ((0, 1, 256, 777), (0, 1, 255, 777 - 3), (0, 1, 1, 4), (0, 2, 776, 776), (0, 2, 777, 777),
                                      (0, 4, 500, 500), (0, 4, 778, 777), (2, 2, 1, 777), (1, 1, 3, 768), (1, 1, 2, 512)):
        a = vm.add_map(MapDef(MAP_ARRAY, 4, 8, entries))
        ref.add_map(MapDef(MAP_ARRAY, 4, 8, entries))
        fill(vm, ref, a, dev, array_rows(entries), rng.integers(1, 256, size=(entries, 8), dtype=np.uint8))
        for mode in MODES:
            _, _, matched, _ = check_join(lib, vm, ref, src, a, dev, MapJoin(MG_KEY, off, ln, mode), snap=snap, cap=9)
            assert matched == (present if mode == MJ_PRESENT else 777 - present), (off, ln, entries, mode)
    vm.close()
    ref.close()
    # a HASH source against ARRAYs, by a value byte and by two value bytes at an odd offset
    vm, ref, src, a1 = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 16, 16, 1024), MapDef(MAP_ARRAY, 4, 24, 100))
    a2 = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 30000))
    ref.add_map(MapDef(MAP_ARRAY, 4, 8, 30000))
    SC.fill_hash(vm, ref, src, dev, rng, 16, 16, 900)
    fill(vm, ref, a1, dev, array_rows(100), rng.integers(1, 256, size=(100, 24), dtype=np.uint8))
    snap = Snapshot(vm, ref, src, dev)
    for mode in MODES:
        _, _, m1, sel = check_join(lib, vm, ref, src, a1, dev, MapJoin(MG_KEY, 9, 1, mode), snap=snap)
        _, _, m2, _ = check_join(lib, vm, ref, src, a2, dev, MapJoin(MG_VALUE, 13, 2, mode), snap=snap, cap=20)
        assert sel == 600 and 0 < m1 < 600 and 0 < m2 < 600
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 7. filters
def run_filters(lib, oracle_lib, dev) -> None:
    """Every filter op combined with the join: selected is the scan's count for the same filter."""
    rng = np.random.default_rng(707)
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 13, 24, MC.HASH_MAX), MapDef(MAP_HASH, 1, 8, 256))
    SC.fill_hash(vm, ref, src, dev, rng, 13, 24, 60)
    fill(vm, ref, other, dev, np.arange(0, 256, 2, dtype=np.uint8).reshape(-1, 1), rng.integers(1, 256, size=(128, 8), dtype=np.uint8))
    snap = Snapshot(vm, ref, src, dev)
    live = len(snap.keys)
    operand = int(fields(snap.vals, 16, 8)[live // 2])
    total = {}
    for op in SC.OPS:
        flt = MapFilter(op, 16, 8, operand)
        scanned = SC.raw_call(lib, vm, src, flt, 0, 0, 0, True, False)
        kept = 0
        for mode in MODES:
            _, _, matched, selected = check_join(lib, vm, ref, src, other, dev, MapJoin(MG_KEY, 4, 1, mode), flt, snap=snap)
            assert (0, selected) == scanned
            kept += matched
        assert kept == selected  # present and absent split the candidates
        total[op] = selected
    assert total[SC.ALL] == live and total[EQ] == 1 and total[NE] == live - 1 and total[SC.GE] + total[SC.LT] == live
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 8. removal
def run_removal(lib, oracle_lib, dev, host_form: bool = False) -> None:
    """Apply a blocklist: reported with cap_entries below matched (exactly the first r go), silently, then the rest;
    the count, a following lookup, and re-inserting the removed keys takes their records again."""
    rng = np.random.default_rng(808)
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 16, 40, 256), MapDef(MAP_HASH, 4, 8, 64))
    n = 200
    keys = hash_pool(rng, 16, n)
    addrs = hash_pool(rng, 4, 30)
    keys[:, 3:7] = addrs[rng.integers(0, 30, size=n)]
    keys = np.unique(keys, axis=0)
    n = len(keys)
    vals = rng.integers(1, 256, size=(n, 40), dtype=np.uint8)
    fill(vm, ref, src, dev, keys, vals)
    fill(vm, ref, other, dev, addrs[:12], rng.integers(1, 256, size=(12, 8), dtype=np.uint8))
    j = MapJoin(MG_KEY, 3, 4, MJ_PRESENT)
    first = Snapshot(vm, ref, src, dev)
    ek, r, matched, _ = check_join(lib, vm, ref, src, other, dev, j, cap=7, rm=True, host_form=host_form, snap=first)
    assert r == 7 < matched
    for i, k in enumerate(ek):  # exactly those r keys are gone, every other match is still there
        assert (vm.map_lookup(src, k.tobytes()) is None) == (i < r)
    vm.map_update(src, ek[0].tobytes(), b"\x11" * 40)  # (a host visit drops the tombstones; one blocked entry is back)
    ref.map_update(src, ek[0].tobytes(), b"\x11" * 40)
    # silently: no output at all, up to cap_entries of them
    ek2, r2, matched2, _ = check_join(lib, vm, ref, src, other, dev, j, cap=5, rm=True, outs=(False, False, False), host_form=host_form)
    assert (r2, matched2) == (5, matched - 6)
    # the rest, values alone
    ek3, r3, matched3, _ = check_join(lib, vm, ref, src, other, dev, j, rm=True, outs=(False, True, True), host_form=host_form)
    assert r3 == matched3 == matched2 - 5
    assert raw_join(lib, vm, src, None, j, other) == (0, 0, n - matched)
    assert vm.map_count(src) == ref.map_count(src) == n - matched
    same_map(vm, ref, src, "after the blocklist")
    # the removed keys come back: each takes its old record again (no host visit in between)
    before = Snapshot(vm, ref, src, dev)
    ek4, r4, _, _ = check_join(lib, vm, ref, src, other, dev, MapJoin(MG_KEY, 3, 4, MJ_ABSENT), cap=20, rm=True, host_form=host_form,
                               snap=before)
    assert r4 == 20
    ek4 = ek4[:20]
    nv = rng.integers(1, 256, size=(20, 40), dtype=np.uint8)
    vm.map_update_batch_device(src, dev(np.ascontiguousarray(ek4)), dev(nv))
    MC.ref_update(ref, src, ek4, nv)
    after = Snapshot(vm, ref, src, dev)
    assert after.tombs == before.tombs and np.array_equal(after.slots, before.slots), "a key that came back did not take its old record"
    same_image_map(vm, ref, src, dev, "removed keys installed again")
    vm.close()
    ref.close()


def run_removal_delta(lib, dev) -> None:
    """The delta base goes to zero with the removed values: xe_map_delta reports nothing on the removed records."""
    vm, m = flow_vm(lib)
    block = vm.add_map(MapDef(MAP_HASH, 16, 8, 64))
    keys, vals = MC.flow_entries(list(range(40)))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    vm.map_update_batch_device(block, dev(np.ascontiguousarray(keys[5:15])), dev(np.ones((10, 8), np.uint8)))
    traffic = vm.map_traffic(m), vm.map_traffic(block)
    k, v, matched, selected = vm.map_join(m, block, MapJoin(MG_KEY, 0, 16, MJ_PRESENT), remove=True, on_device=on_dev(dev(keys[:1])))
    assert (matched, selected) == (10, 40)
    assert {bytes(x) for x in to_np(k)} == {bytes(x) for x in keys[5:15]}
    out = dev(np.full(vm.map_values_bytes(m), GUARD, np.uint8))
    settle(out)
    vm.map_delta(m, addr(out), lane=8)
    assert not to_np(out)[:(MC.hash_geometry(vm, m)[0] + 1) * 16].any(), "a removal left the delta base behind"
    assert (vm.map_traffic(m), vm.map_traffic(block)) == traffic, "a join moved a whole map"
    assert vm.map_count(m) == 30
    vm.close()


# ---------------------------------------------------------------- 9. self-join
def run_self_join(lib, oracle_lib, dev) -> None:
    """Sessions that name a parent session of the same map in their value: which parents are gone (ABSENT), their
    removal, and the parents' values beside the children (PRESENT with the third output)."""
    rng = np.random.default_rng(909)
    n = 300
    vm, ref, m, _ = MC.pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 20, 1024))
    keys = hash_pool(rng, 8, n + 40)
    vals = rng.integers(0, 256, size=(n + 40, 20), dtype=np.uint8)
    vals[:, 3:11] = keys[rng.integers(0, n + 40, size=n + 40)]  # the parent: any key, 40 of which are deleted below
    fill(vm, ref, m, dev, keys, vals)
    remove(vm, ref, m, dev, keys[n:])
    snap = Snapshot(vm, ref, m, dev)
    _, _, have, selected = check_join(lib, vm, ref, m, m, dev, MapJoin(MG_VALUE, 3, 8, MJ_PRESENT), snap=snap)
    _, _, orphans, _ = check_join(lib, vm, ref, m, m, dev, MapJoin(MG_VALUE, 3, 8, MJ_ABSENT), snap=snap, cap=4)
    assert selected == n == have + orphans and orphans >= 10
    # by its own key every entry is present, and the third output is the second
    ek, r, matched, _ = check_join(lib, vm, ref, m, m, dev, MapJoin(MG_KEY, 0, 8, MJ_PRESENT), snap=snap)
    assert matched == n
    # removal: the orphans go; the values reported (the removed entries' own, and zeros for the absent parents) are
    # those from before the removal. Removing them orphans more: the oracle agrees on every round
    rounds = 0
    while True:
        _, r, matched, _ = check_join(lib, vm, ref, m, m, dev, MapJoin(MG_VALUE, 3, 8, MJ_ABSENT), rm=True)
        if not matched:
            break
        rounds += 1
    assert rounds >= 1
    # present with removal: every entry whose parent is there goes, parents included, and the parents' values that
    # are reported are those from before any of them was removed
    check_join(lib, vm, ref, m, m, dev, MapJoin(MG_VALUE, 3, 8, MJ_PRESENT), rm=True)
    same_map(vm, ref, m, "after the self-joins")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 10. beside traffic
def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    """A pipelined batch is in flight when the join is called: the call completes it itself and its answer is the
    one a call after xe_sync gives."""
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    odef = MapDef(MAP_HASH, 4, 16, 256)
    other = vm.add_map(odef)
    assert ref.add_map(odef) == other and rm == m
    r = Runner(vm, dev, use_async)
    keys, vals = MC.flow_entries(list(range(48)))
    install(vm, ref, m, dev, keys, vals)
    srcs = np.unique(keys[:, 0:4], axis=0)
    install(vm, ref, other, dev, np.ascontiguousarray(srcs[::2]), np.full((len(srcs[::2]), 16), 9, np.uint8))
    v0 = r.run(0)
    umem, descs = MC.W.build_batch("c3learn", 0, MC.FLOW_PACKETS)
    w0 = ref.run_batch(umem, descs).verdicts
    j = MapJoin(MG_KEY, 0, 4, MJ_ABSENT)
    room = MC.FLOW_MAX
    bufs = [dev(np.full((room, w), GUARD, np.uint8)) for w in (16, 16, 16)]
    for b in bufs:
        settle(b)
    rc, matched, selected = raw_join(lib, vm, m, None, j, other, *[addr(b) for b in bufs], cap=room)  # completes the pipeline itself
    assert rc == 0, lib.last_error(vm.h)
    assert np.array_equal(to_np(v0), w0)
    snap = Snapshot(vm, ref, m, dev)  # (after xe_sync; the join changed nothing)
    ek, ev, eo, ncand = expect_join(snap, ref, other, j, None)
    assert (matched, selected) == (len(ek), ncand) and ncand == ref.map_count(rm) > 48 and 0 < matched < ncand
    assert np.array_equal(to_np(bufs[0])[:matched], ek) and np.array_equal(to_np(bufs[1])[:matched], ev)
    assert not to_np(bufs[2])[:matched].any()
    check_join(lib, vm, ref, m, other, dev, j, snap=snap)  # the same call after the sync: the same answer
    # a host write to either map, then a join: each is uploaded exactly once
    nk, _ = MC.flow_entries([1 << 40])
    vm.map_update(m, nk[0].tobytes(), b"\x01" * 16)
    ref.map_update(rm, nk[0].tobytes(), b"\x01" * 16)
    vm.map_update(other, nk[0, 0:4].tobytes(), b"\x02" * 16)
    ref.map_update(other, nk[0, 0:4].tobytes(), b"\x02" * 16)
    up = vm.map_traffic(m)[0], vm.map_traffic(other)[0]
    check_join(lib, vm, ref, m, other, dev, MapJoin(MG_KEY, 0, 4, MJ_PRESENT), MapFilter(EQ, 0, 8, 0x0101010101010101))
    assert raw_join(lib, vm, m, None, j, other)[0] == 0
    assert (vm.map_traffic(m)[0], vm.map_traffic(other)[0]) == (up[0] + 1, up[1] + 1)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 11. epoch
def run_epoch(lib, dev) -> None:
    vm, m = flow_vm(lib)
    other = vm.add_map(MapDef(MAP_HASH, 16, 8, 64))
    keys, vals = MC.flow_entries(range(8))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    vm.map_update_batch_device(other, dev(np.ascontiguousarray(keys[:3])), dev(np.ones((3, 8), np.uint8)))
    j = MapJoin(MG_KEY, 0, 16, MJ_PRESENT)
    vm.epoch_begin()
    for device_form in (True, False):
        assert raw_join(lib, vm, m, None, j, other, cap=8, flags=MJ_REMOVE, device_form=device_form)[0] == MC.ERR_INVAL
        assert raw_join(lib, vm, m, None, j, other, cap=8, device_form=device_form) == (0, 3, 8)  # a report is allowed
    k, v, matched, selected = vm.map_join(m, other, j)
    assert (matched, selected) == (3, 8) and {bytes(x) for x in k} == {bytes(x) for x in keys[:3]}
    vm.epoch_end()
    assert raw_join(lib, vm, m, None, j, other, cap=2, flags=MJ_REMOVE) == (0, 3, 8)  # silently: no output buffers
    assert vm.map_count(m) == 6
    vm.close()


# ---------------------------------------------------------------- 12. limits
def run_limits(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(1212)
    good = N.MapJoin(MG_VALUE, 0, 4, MJ_PRESENT, 0, 0)
    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        bad = vm.add_map(MapDef(t, 4, 16, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 16, 16))
        ok = vm.add_map(MapDef(MAP_HASH, 4, 16, 16))
        for s, d in ((bad, ok), (ok, bad)):
            for device_form in (True, False):
                assert raw_join(lib, vm, s, None, good, d, device_form=device_form)[0] == MC.ERR_UNSUPPORTED, (t, s, d)
                assert b"ARRAY and HASH" in lib.last_error(vm.h)
        vm.close()

    svs = 13
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, svs, MC.HASH_MAX), MapDef(MAP_HASH, 4, 24, MC.HASH_MAX))
    asrc = vm.add_map(MapDef(MAP_ARRAY, 4, svs, 10))
    aoth = vm.add_map(MapDef(MAP_ARRAY, 4, 24, 300))
    nokey = vm.add_map(MapDef(MAP_HASH, 0, 16, 16))
    for d in (MapDef(MAP_ARRAY, 4, svs, 10), MapDef(MAP_ARRAY, 4, 24, 300), MapDef(MAP_HASH, 0, 16, 16)):
        ref.add_map(d)
    SC.fill_hash(vm, ref, src, dev, rng, 8, svs, 30)
    snap = Snapshot(vm, ref, src, dev)
    fill(vm, ref, other, dev, np.ascontiguousarray(snap.keys[:5, 0:4]), rng.integers(0, 256, size=(5, 24), dtype=np.uint8))
    before = state_image(vm, src, dev), state_image(vm, other, dev), state_image(vm, aoth, dev), state_image(vm, asrc, dev)
    J, K, V, RM = N.MapJoin, MG_KEY, MG_VALUE, MJ_REMOVE
    #           from off len mode flags pad
    bad = [(src, other, None),                          # j NULL
           (src, other, J(2, 0, 4, 0, 0, 0)),           # from
           (src, other, J(0xffffffff, 0, 4, 0, 0, 0)),
           (src, other, J(K, 0, 4, 2, 0, 0)),           # mode
           (src, other, J(K, 0, 4, 0xffffffff, 0, 0)),
           (src, other, J(K, 0, 4, 0, 2, 0)),           # an unknown flag bit
           (src, other, J(K, 0, 4, 0, RM | 0x80000000, 0)),
           (src, other, J(K, 0, 4, 0, 0, 1)),           # pad
           (src, other, J(K, 5, 4, 0, 0, 0)),           # join bytes outside the 8-byte key
           (src, other, J(K, 0xfffffffe, 4, 0, 0, 0)),
           (src, other, J(V, svs - 3, 4, 0, 0, 0)),     # ... outside the value
           (asrc, other, J(K, 1, 4, 0, 0, 0)),          # ... outside an ARRAY source's four index bytes
           (src, other, J(K, 0, 3, 0, 0, 0)),           # len != the other map's key_size
           (src, other, J(K, 0, 8, 0, 0, 0)),
           (src, aoth, J(K, 0, 3, 0, 0, 0)),            # an ARRAY other map: len 1, 2 or 4
           (src, aoth, J(K, 0, 0, 0, 0, 0)),
           (src, aoth, J(K, 0, 8, 0, 0, 0)),
           (src, nokey, J(K, 0, 0, 0, 0, 0)),           # a HASH other map without key bytes
           (asrc, other, J(K, 0, 4, 0, RM, 0)),         # removal from an ARRAY source
           (asrc, aoth, J(K, 0, 4, 1, RM, 0))]
    k3 = [np.zeros(64 * 64, np.uint8) for _ in range(3)]
    for s, d, j in bad:
        what = None if j is None else tuple(getattr(j, f[0]) for f in j._fields_)
        for device_form in (True, False):
            rc = raw_join(lib, vm, s, None, j, d, *[b.ctypes.data for b in k3], cap=5, device_form=device_form)[0]
            assert rc == MC.ERR_INVAL, (s, d, what, rc)
    ok = J(K, 0, 4, 0, 0, 0)
    for device_form in (True, False):
        assert raw_join(lib, vm, src, None, ok, other, matched=False, device_form=device_form)[0] == MC.ERR_INVAL  # a NULL matched
        for f in (N.MapFilter(9, 0, 1, 0, 0), N.MapFilter(EQ, 0, 1, 1, 0), N.MapFilter(EQ, 0, 3, 0, 0), N.MapFilter(EQ, svs, 1, 0, 0)):
            assert raw_join(lib, vm, src, f, ok, other, device_form=device_form)[0] == MC.ERR_INVAL  # the scan's filter errors
        assert raw_join(lib, vm, 99, None, ok, other, device_form=device_form)[0] == MC.ERR_INVAL  # a bad map index
        assert raw_join(lib, vm, src, None, ok, 99, device_form=device_form)[0] == MC.ERR_INVAL
    assert not any(b.any() for b in k3), "a refused call wrote an output"
    after = state_image(vm, src, dev), state_image(vm, other, dev), state_image(vm, aoth, dev), state_image(vm, asrc, dev)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused call changed a map"
    same_map(vm, ref, src, "after the refused calls")
    same_map(vm, ref, other, "after the refused calls")
    # a NULL selected is allowed; cap_entries 0 with buffers, and a removal with cap_entries 0, only count
    now = state_image(vm, src, dev)  # (the dump above was a host visit: the tombstones are gone)
    rc, matched, _ = raw_join(lib, vm, src, None, ok, other, selected=False)
    assert (rc, matched) == (0, 5)
    assert raw_join(lib, vm, src, None, ok, other, *[b.ctypes.data for b in k3], cap=0) == (0, 5, 20)
    assert raw_join(lib, vm, src, None, ok, other, cap=0, flags=RM) == (0, 5, 20)
    assert not any(b.any() for b in k3) and np.array_equal(now, state_image(vm, src, dev))
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 13. the Python interface
def run_python_api(lib, oracle_lib, dev, on_device: bool) -> None:
    rng = np.random.default_rng(1313)
    vm, ref, src, other = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, MC.HASH_MAX), MapDef(MAP_HASH, 2, 24, 64))
    SC.fill_hash(vm, ref, src, dev, rng, 8, 16, 40, delete_third=False)
    snap = Snapshot(vm, ref, src, dev)
    fill(vm, ref, other, dev, np.ascontiguousarray(snap.vals[::2, 5:7]), rng.integers(1, 256, size=(20, 24), dtype=np.uint8))
    flt = MapFilter(ANYBITS, 0, 1, 0x3f)
    j = MapJoin(MG_VALUE, 5, 2, MJ_PRESENT)
    ek, ev, eo, ncand = expect_join(snap, ref, other, j, flt)
    assert 5 <= len(ek) < ncand < 40
    k, v, matched, selected = vm.map_join(src, other, j, flt, on_device=on_device)  # cap None: count first, then fetch all
    assert on_dev(k) == on_device and (matched, selected) == (len(ek), ncand)
    assert np.array_equal(to_np(k), ek) and np.array_equal(to_np(v), ev)
    k, v, o, matched, selected = vm.map_join(src, other, j, flt, cap=3, on_device=on_device, other_values=True)
    assert (matched, selected) == (len(ek), ncand) and on_dev(o) == on_device
    assert np.array_equal(to_np(k), ek[:3]) and np.array_equal(to_np(v), ev[:3]) and np.array_equal(to_np(o), eo[:3])
    ak, av, aeo, _ = expect_join(snap, ref, other, MapJoin(MG_VALUE, 5, 2, MJ_ABSENT), None)
    k, v, o, matched, selected = vm.map_join(src, other, MapJoin(MG_VALUE, 5, 2, MJ_ABSENT), on_device=on_device, remove=True,
                                             other_values=True)
    assert (matched, selected) == (len(ak), 40) and np.array_equal(to_np(k), ak) and np.array_equal(to_np(v), av) and not to_np(o).any()
    MC.ref_delete(ref, src, ak)
    same_image_map(vm, ref, src, dev, "after VM.map_join(remove=True)")
    same_map(vm, ref, src, "after VM.map_join(remove=True)")
    vm.close()
    ref.close()
