"""Shared cases of the device-side map scan and expire (xe_map_scan_device / xe_map_expire_device and
their host-pointer forms): tests/test_mapscan.py runs them on the host simulation,
tests/test_mapscan_gpu.py on the product library.

No expected value comes from the code under test:
  * the SET of selected entries is the oracle VM's map_dump, filtered by `predicate`, a numpy restatement
    of the nine filter ops that is itself pinned by a table of hand-computed triples (PREDICATE_TABLE);
  * the ORDER is the FULL records of the exported state image (mapops_cases.state_image: device to
    device, no host visit) in slot order, filtered the same way; for an ARRAY map, the index order;
  * after an expire the oracle deletes the same keys one by one, and the maps are compared through the
    image (same_image_map), the dump (same_map) and map_count.

`dev` turns a numpy array into what a call is given for device memory: the array itself on the host
simulation, a CUDA tensor on the product; a numpy array given to the product goes through the
host-pointer forms (xe_map_scan / xe_map_expire).

The sizes come from the kernels' constants (xe_mapops.h): a tile is kMsTile = 256 consecutive slots, one
wave's work in kMsRounds = 4 rounds of 64; the SCAN step sums kMsScanPass = 1,024 tile counts a pass, so a
table of more than 262,144 slots needs its carry (a HASH table has the next power of two >= 2 x
max_entries slots, at least 16). The value sub-groups (xe_mo_lanes) cut at 16, 64 and 1,024 bytes, the
record sizes at 0, 8, 24 and 56 key bytes, as in mapops_cases.EDGE_PAIRS."""
from __future__ import annotations

import ctypes as C

import numpy as np

import mapops_cases as MC
from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, VM, MapDef,
                                  MapFilter, Settings)
from mapops_cases import (GUARD, addr, flow_vm, guards_intact, hash_pool, image_records, on_dev, pair, place, same_image_map,
                          same_map, settle, state_image, to_np, Runner)

ALL, EQ, NE, LT, LE, GT, GE, ANYBITS, NOBITS = range(9)  # include/xdpemu.h XE_MF_*
OPS = (ALL, EQ, NE, LT, LE, GT, GE, ANYBITS, NOBITS)
M64 = (1 << 64) - 1
TILE, SCAN_PASS = 256, 1024  # xe_mapops.h kMsTile, kMsScanPass

MATRIX_KEY_SIZES = (0, 8, 13, 16, 17, 24, 25, 56, 64)
MATRIX_VALUE_SIZES = (1, 8, 16, 17, 64, 65, 1024, 1025, 4096)
MATRIX_PAIRS = tuple(dict.fromkeys([(ks, vs) for vs in MATRIX_VALUE_SIZES for ks in (8, 24)] +
                                   [(ks, vs) for ks in MATRIX_KEY_SIZES for vs in (8, 65)]))
ARRAY_VALUE_SIZES = (1, 24, 65, 1025)
ARRAY_ENTRIES = (1, 100, 4099)  # below a wave; below a tile; 17 tiles, the last one partial
ALIGN_OFFSETS = (0, 1, 4, 8)
ALIGN_PAIRS = ((8, 8), (16, 64), (24, 100), (8, 4097))


# ---------------------------------------------------------------- the nine predicates, restated
def predicate(op: int, field: np.ndarray, operand: int) -> np.ndarray:
    """Which of the zero-extended fields (uint64) the filter selects."""
    f, o = np.asarray(field, dtype=np.uint64), np.uint64(operand)
    if op == ALL:
        return np.ones(len(f), dtype=bool)
    if op == EQ:
        return f == o
    if op == NE:
        return f != o
    if op == LT:
        return f < o
    if op == LE:
        return f <= o
    if op == GT:
        return f > o
    if op == GE:
        return f >= o
    if op == ANYBITS:
        return (f & o) != 0
    if op == NOBITS:
        return (f & o) == 0
    raise ValueError(op)


# (op, field, operand, selected), worked out by hand; the compares are unsigned over 64 bits
PREDICATE_TABLE = (
    (ALL, 0, 5, True), (ALL, M64, 0, True),
    (EQ, 7, 7, True), (EQ, 7, 8, False), (EQ, 0xff, 0x1ff, False), (EQ, 0, 0, True),
    (NE, 7, 7, False), (NE, 7, 8, True), (NE, 0xff, 0x100, True),
    (LT, 7, 7, False), (LT, 6, 7, True), (LT, 8, 7, False), (LT, 1, 1 << 63, True), (LT, 1 << 63, 1, False),
    (LT, 0xffff, 0x10000, True), (LT, 0, 0, False),
    (LE, 7, 7, True), (LE, 8, 7, False), (LE, M64, M64, True), (LE, 1 << 63, (1 << 63) - 1, False),
    (GT, 7, 7, False), (GT, 8, 7, True), (GT, 1 << 63, 1, True), (GT, 1, 1 << 63, False), (GT, M64, M64 - 1, True),
    (GE, 7, 7, True), (GE, 6, 7, False), (GE, 0, 0, True), (GE, (1 << 63) - 1, 1 << 63, False),
    (ANYBITS, 0b1010, 0b0100, False), (ANYBITS, 0b1010, 0b0010, True), (ANYBITS, 0, M64, False), (ANYBITS, 1 << 63, M64, True),
    (ANYBITS, 5, 0, False),
    (NOBITS, 0b1010, 0b0100, True), (NOBITS, 0b1010, 0b0010, False), (NOBITS, 0, M64, True), (NOBITS, 1 << 63, M64, False),
    (NOBITS, 5, 0, True),
)


def check_predicate_table() -> None:
    for op, field, operand, want in PREDICATE_TABLE:
        assert bool(predicate(op, np.array([field], dtype=np.uint64), operand)[0]) is want, (op, field, operand)


def fields(vals: np.ndarray, off: int, width: int) -> np.ndarray:
    """The little-endian unsigned field of `width` bytes at byte `off` of every value."""
    out = np.zeros(len(vals), dtype=np.uint64)
    for b in range(width):
        out |= vals[:, off + b].astype(np.uint64) << np.uint64(8 * b)
    return out


def selects(vals: np.ndarray, flt: MapFilter | None) -> np.ndarray:
    if flt is None or flt.op == ALL:
        return np.ones(len(vals), dtype=bool)
    return predicate(flt.op, fields(vals, flt.offset, flt.width), flt.operand)


# ---------------------------------------------------------------- what a scan must report
class Snapshot:
    """The entries of a map's current state: in slot order from the exported image (HASH) or in index
    order from the oracle's dump (ARRAY), after checking that they are the oracle's entries as a set.
    Taken once per state; a scan changes none."""

    def __init__(self, vm: VM, ref: VM, m: int, dev):
        d = vm.map_defs[m]
        self.array = d.type == MAP_ARRAY
        if self.array:
            raw = np.frombuffer(ref.map_dump(m), dtype=np.uint8)
            self.vals = raw.reshape(d.max_entries, d.value_size).copy()
            self.keys = np.arange(d.max_entries, dtype=np.uint32).view(np.uint8).reshape(-1, 4).copy()
            self.ref_keys, self.ref_vals = self.keys, self.vals
            self.tombs = 0
            return
        w0, keys, vals, count = image_records(vm, m, state_image(vm, m, dev))
        full = np.nonzero(w0 & np.uint64(MC.SLOT_FULL))[0]
        self.keys, self.vals = keys[full].copy(), vals[full].copy()
        self.vals[(w0[full] & np.uint64(MC.SLOT_VLEN0)) != 0] = 0
        self.slots = full
        self.tombs = int(((w0 & np.uint64(MC.SLOT_TOMB)) != 0).sum())
        self.ref_keys, self.ref_vals = ref.map_dump(m)
        assert count == len(full) == len(self.ref_keys) == ref.map_count(m)
        gk, gv = MC.by_key(self.keys, self.vals)
        wk, wv = MC.by_key(self.ref_keys, self.ref_vals)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), "the image's FULL records are not the oracle's entries"

    def expect(self, flt: MapFilter | None):
        """(keys, values) the filter selects, in the order a scan reports them. The set is the oracle's."""
        sel, rsel = selects(self.vals, flt), selects(self.ref_vals, flt)
        k, v = self.keys[sel], self.vals[sel]
        gk, gv = MC.by_key(k, v)
        wk, wv = MC.by_key(self.ref_keys[rsel], self.ref_vals[rsel])
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
        return k, v


def raw_call(lib, vm: VM, m: int, flt, kptr, vptr, cap: int, device_form: bool, expire: bool, matched=True):
    """One call by address. Returns (rc, matched)."""
    cf = None if flt is None else (flt if isinstance(flt, N.MapFilter) else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand))
    n = C.c_uint64(0xDEADBEEF)
    head = (vm.h, m, None if cf is None else C.byref(cf), kptr or None, vptr or None, cap, C.byref(n) if matched else None)
    if device_form:
        rc = (lib.map_expire_device if expire else lib.map_scan_device)(*head, None)
    else:
        rc = (lib.map_expire if expire else lib.map_scan)(*head)
    return rc, n.value


def call(lib, vm: VM, m: int, dev, flt, cap: int, room: int, expire: bool = False, koff: int = 0, voff: int = 0,
         want_keys: bool = True, want_vals: bool = True, host_form: bool = False):
    """A scan or an expire into GUARD buffers of `room` entries, `koff` / `voff` bytes past a 16-byte
    boundary. Returns (keys[r], values[r], matched, the two whole buffers on the host) after checking that
    no byte in front of the buffers or behind entry r was written."""
    d = vm.map_defs[m]
    ks, vs = (4 if d.type == MAP_ARRAY else d.key_size), d.value_size
    mk = np.ascontiguousarray if host_form else dev  # host memory for the host-pointer forms
    kbuf, _ = place(mk, np.full((room, ks), GUARD, np.uint8), koff)
    vbuf, _ = place(mk, np.full((room, vs), GUARD, np.uint8), voff)
    settle(kbuf)
    settle(vbuf)
    device_form = not host_form
    rc, matched = raw_call(lib, vm, m, flt, addr(kbuf) + koff if want_keys else 0, addr(vbuf) + voff if want_vals else 0, cap,
                           device_form, expire)
    assert rc == 0, lib.last_error(vm.h)
    r = min(matched, cap)
    assert r <= room
    what = f"{'expire' if expire else 'scan'} cap {cap}, keys +{koff}, values +{voff}"
    k = guards_intact(kbuf, koff, r * ks if want_keys else 0, what + ": keys").reshape(-1, ks) if ks else np.zeros((r, 0), np.uint8)
    if not ks:
        guards_intact(kbuf, koff, 0, what + ": keys")
    v = guards_intact(vbuf, voff, r * vs if want_vals else 0, what + ": values").reshape(-1, vs)
    return k, v, matched, (to_np(kbuf).copy(), to_np(vbuf).copy())


def check_scan(lib, vm, snap: Snapshot, m, dev, flt, cap=None, extra_room: int = 3, **kw):
    """A scan against the snapshot: the total, the first r entries of the expected order, the guards."""
    ek, ev = snap.expect(flt)
    cap = len(ek) if cap is None else cap
    k, v, matched, _ = call(lib, vm, m, dev, flt, cap, min(cap, len(ek)) + extra_room, **kw)
    r = min(cap, len(ek))
    assert matched == len(ek), f"matched {matched}, expected {len(ek)}"
    if kw.get("want_keys", True):
        assert np.array_equal(k, ek[:r]), "keys differ (or their order)"
    if kw.get("want_vals", True):
        assert np.array_equal(v, ev[:r]), "values differ (or their order)"
    return ek, ev, r


def check_expire(lib, vm, ref, m, dev, flt, cap=None, host_visit: bool = True, **kw):
    """An expire against the state before it: what it reports, then the oracle deletes the same keys one by
    one and the maps must agree; the removed records are plain tombstones that kept their key words, with
    zero values. Returns (expected keys, r)."""
    before = Snapshot(vm, ref, m, dev)
    ek, ev = before.expect(flt)
    cap = len(ek) if cap is None else cap
    r = min(cap, len(ek))
    k, v, matched, _ = call(lib, vm, m, dev, flt, cap, r + 3, expire=True, **kw)
    assert matched == len(ek), f"matched {matched}, expected {len(ek)}"
    if kw.get("want_keys", True):
        assert np.array_equal(k, ek[:r]), "keys differ (or their order)"
    if kw.get("want_vals", True):
        assert np.array_equal(v, ev[:r]), "values differ: the values before the removal are reported"
    MC.ref_delete(ref, m, ek[:r])
    img = same_image_map(vm, ref, m, dev, "after the expire")
    w0, keys, vals, count = image_records(vm, m, img)
    gone = before.slots[selects(before.vals, flt)][:r]
    assert (w0[gone] == np.uint64(MC.SLOT_TOMB)).all(), "a removed record is not a plain tombstone"
    assert np.array_equal(keys[gone], ek[:r]), "a removed record lost its key words"
    assert not vals[gone].any(), "a removed record's value is not zero"
    assert count == len(before.keys) - r
    assert int(((w0 & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == before.tombs + r
    rest = raw_call(lib, vm, m, flt, 0, 0, 0, True, False)
    assert rest == (0, len(ek) - r), "a second call does not report the matches left"
    if host_visit:
        same_map(vm, ref, m, "after the expire")
        assert vm.map_count(m) == ref.map_count(m) == len(before.keys) - r
    return ek, r


def fill_hash(vm, ref, m, dev, rng, ks: int, vs: int, n: int, delete_third: bool = True):
    """n random entries; a third of them deleted again through map_delete_batch: live tombstones."""
    keys = hash_pool(rng, ks, n)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, m, keys, vals)
    if delete_third:
        gone = np.ascontiguousarray(keys[::3])
        assert to_np(vm.map_delete_batch(m, dev(gone))).all()
        MC.ref_delete(ref, m, gone)
    return keys, vals


def widest(vs: int) -> int:
    return 8 if vs >= 8 else 4 if vs >= 4 else 2 if vs >= 2 else 1


def every_op(lib, vm, snap: Snapshot, m, dev, vs: int, **kw) -> None:
    """Every op once with an operand taken from a present value, and with that operand + 1 and - 1."""
    width = widest(vs)
    off = vs - width
    live = len(snap.keys)
    assert live >= 1
    present = int(fields(snap.ref_vals, off, width)[len(snap.ref_vals) // 2])
    for operand in (present, (present + 1) & M64, (present - 1) & M64):
        count = {}
        for op in OPS:
            ek, _, _ = check_scan(lib, vm, snap, m, dev, MapFilter(op, off, width, operand), **kw)
            count[op] = len(ek)
        # what the case names, on the oracle's side: complementary ops split the live entries
        assert count[ALL] == live
        assert count[EQ] + count[NE] == count[LT] + count[GE] == count[LE] + count[GT] == count[ANYBITS] + count[NOBITS] == live
        assert count[LE] == count[LT] + count[EQ]
        if operand == present:
            assert count[EQ] >= 1 and count[LE] >= 1 and count[GE] >= 1


# ---------------------------------------------------------------- 1. matrix
def run_hash_matrix(lib, oracle_lib, dev, ks: int, vs: int, host_form: bool = False) -> None:
    if ks == 0:
        return run_empty_key(lib, oracle_lib, dev, vs, host_form)
    rng = np.random.default_rng(2000 * ks + vs)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    fill_hash(vm, ref, m, dev, rng, ks, vs, MC.HASH_MAX // 2)
    snap = Snapshot(vm, ref, m, dev)
    assert snap.tombs == 11 and len(snap.keys) == 21  # 32 installed, every third deleted
    every_op(lib, vm, snap, m, dev, vs, host_form=host_form)
    check_expire(lib, vm, ref, m, dev, MapFilter(ANYBITS, vs - 1, 1, 1), host_form=host_form)
    vm.close()
    ref.close()


def run_array_matrix(lib, oracle_lib, dev, vs: int, entries: int, host_form: bool = False) -> None:
    rng = np.random.default_rng(3000 * vs + entries)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, entries))
    idx = np.ascontiguousarray(rng.permutation(entries)[: (entries + 1) // 2].astype(np.uint32))
    vals = rng.integers(0, 256, size=(len(idx), vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(idx.view(np.uint8).reshape(-1, 4)), dev(vals))
    MC.ref_update(ref, m, idx.view(np.uint8).reshape(-1, 4), vals)
    snap = Snapshot(vm, ref, m, dev)
    assert len(snap.keys) == entries
    every_op(lib, vm, snap, m, dev, vs, host_form=host_form)
    # keys alone, values alone
    check_scan(lib, vm, snap, m, dev, None, want_vals=False, host_form=host_form)
    check_scan(lib, vm, snap, m, dev, None, want_keys=False, host_form=host_form)
    same_map(vm, ref, m, "ARRAY after the scans")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. slot counts
def hash8(counters: np.ndarray) -> np.ndarray:
    """mapops_cases.hash_words for 8-byte keys (a little-endian counter), vectorised (uint64 wraps)."""
    with np.errstate(over="ignore"):
        h = np.uint64(0x9E3779B97F4A7C15) ^ (np.uint64(8) * np.uint64(0xC2B2AE3D27D4EB4F))
        h = h ^ counters.astype(np.uint64)
        h = h * np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(32)
        h ^= h >> np.uint64(29)
        h = h * np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(32)
    return h


def keys_for_slots(cap: int, n: int) -> np.ndarray:
    """n distinct 8-byte keys (counters): the first two have their home in slot 0 and in slot cap - 1, the
    rest are the first counters that are neither."""
    c = np.arange(1, 8 * max(cap, 1024) + 1, dtype=np.uint64)
    home = (hash8(c) & np.uint64(0xffffffff)) & np.uint64(cap - 1)
    first, last = c[home == 0][:1], c[home == np.uint64(cap - 1)][:1]
    assert len(first) == 1 and len(last) == 1
    for k in (first[0], last[0], c[0], c[12345 % len(c)]):  # the vectorised hash is the restated one
        assert int(hash8(np.array([k]))[0]) == MC.hash_words(int(k).to_bytes(8, "little"))
    rest = c[(c != first[0]) & (c != last[0])][: n - 2]
    return np.ascontiguousarray(np.concatenate([first, last, rest]).view(np.uint8).reshape(-1, 8))


# (max_entries, slots, live keys): 16 slots, below one wave; one tile; two tiles; four passes of the SCAN
# step (2^20 slots = 4,096 tile counts), sparse: 5,000 keys keep the oracle to a few thousand calls.
SLOT_CASES = ((8, 16, 6), (128, TILE, 100), (256, 2 * TILE, 200), (1 << 19, 1 << 20, 5000))
# an ARRAY of one tile plus one slot (a HASH table has a power of two)
ARRAY_TILE_PLUS_ONE = TILE + 1


def run_slot_counts(lib, oracle_lib, dev, max_entries: int, slots: int, live: int, host_form: bool = False) -> None:
    rng = np.random.default_rng(slots)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 8, max_entries))
    assert MC.hash_geometry(vm, m)[0] == slots
    assert slots <= (1 << 20) and ((slots // TILE > SCAN_PASS) == (slots == 1 << 20))
    keys = keys_for_slots(slots, live)
    vals = rng.integers(0, 256, size=(live, 8), dtype=np.uint8)
    vals[:, 7] = 0  # ... so that no value is the one that marks the last slot's entry
    vals[1] = 0xFF
    vm.map_update_batch_device(m, dev(keys[:2].copy()), dev(vals[:2].copy()))  # first: they get their home slots
    vm.map_update_batch_device(m, dev(keys[2:].copy()), dev(vals[2:].copy()))
    MC.ref_update(ref, m, keys, vals)
    snap = Snapshot(vm, ref, m, dev)
    assert snap.slots[0] == 0 and snap.slots[-1] == slots - 1, "the first and the last slot are to be occupied"
    assert np.array_equal(snap.vals[-1], vals[1])
    none = check_scan(lib, vm, snap, m, dev, MapFilter(EQ, 0, 8, 0x00FFFFFFFFFFFFFF), host_form=host_form)
    assert len(none[0]) == 0
    everything = check_scan(lib, vm, snap, m, dev, None, host_form=host_form)
    assert len(everything[0]) == live
    one = check_scan(lib, vm, snap, m, dev, MapFilter(EQ, 0, 8, M64), host_form=host_form)
    assert len(one[0]) == 1 and np.array_equal(one[0][0], keys[1])  # the match in the last slot of the last tile
    half = check_scan(lib, vm, snap, m, dev, MapFilter(ANYBITS, 0, 1, 1), host_form=host_form)
    assert 0.3 * live <= len(half[0]) <= 0.7 * live
    # count only: no buffers at all, and a cap of 0 with buffers
    assert raw_call(lib, vm, m, None, 0, 0, 1 << 40, True, False) == (0, live)
    check_scan(lib, vm, snap, m, dev, MapFilter(ANYBITS, 0, 1, 1), cap=0, host_form=host_form)
    ek, r = check_expire(lib, vm, ref, m, dev, MapFilter(ANYBITS, 0, 1, 1), host_form=host_form)
    assert r == len(half[0])
    vm.close()
    ref.close()


def run_array_tile_plus_one(lib, oracle_lib, dev) -> None:
    vs, entries = 8, ARRAY_TILE_PLUS_ONE
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, entries))
    idx = np.array([0, TILE - 1, TILE], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vals = np.array([[1] * vs, [2] * vs, [3] * vs], dtype=np.uint8)
    vm.map_update_batch_device(m, dev(idx), dev(vals))
    MC.ref_update(ref, m, idx, vals)
    snap = Snapshot(vm, ref, m, dev)
    ek, ev, _ = check_scan(lib, vm, snap, m, dev, MapFilter(NE, 0, 8, 0))
    assert np.array_equal(ek, idx) and np.array_equal(ev, vals)
    ek, _, _ = check_scan(lib, vm, snap, m, dev, MapFilter(EQ, 0, 1, 3))
    assert np.array_equal(ek, idx[2:])  # the one slot of the second tile
    assert len(check_scan(lib, vm, snap, m, dev, None)[0]) == entries
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. cap_entries
def run_caps(lib, oracle_lib, dev, expire: bool, host_form: bool = False) -> None:
    ks, vs = 13, 24
    flt = MapFilter(ANYBITS, 5, 2, 0x0101)
    for which in range(5):
        rng = np.random.default_rng(33)
        vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
        fill_hash(vm, ref, m, dev, rng, ks, vs, 60)
        snap = Snapshot(vm, ref, m, dev)
        matched = len(snap.expect(flt)[0])
        assert 10 <= matched < len(snap.keys)
        cap = (0, 1, matched - 1, matched, matched + 7)[which]
        if not expire:
            check_scan(lib, vm, snap, m, dev, flt, cap=cap, host_form=host_form)
        else:
            ek, r = check_expire(lib, vm, ref, m, dev, flt, cap=cap, host_form=host_form)
            assert r == min(cap, matched)
            # exactly those r keys are gone, every other match is still there (the oracle agrees: check_expire)
            for i, k in enumerate(ek):
                assert (vm.map_lookup(m, k.tobytes()) is None) == (i < r)
        vm.close()
        ref.close()


# ---------------------------------------------------------------- 4. fields
def run_fields(lib, oracle_lib, dev, host_form: bool = False) -> None:
    rng = np.random.default_rng(44)
    ks, vs, n = 8, 13, 48
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys = hash_pool(rng, ks, n)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    vals[0] = 0      # fields of all zeros ...
    vals[1] = 0xFF   # ... and of all ones are present
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, m, keys, vals)
    snap = Snapshot(vm, ref, m, dev)

    def count(op, off, width, operand) -> int:
        return len(check_scan(lib, vm, snap, m, dev, MapFilter(op, off, width, operand), host_form=host_form)[0])

    places = [(w, off) for w in (1, 2, 4, 8) for off in (0, vs - w)] + [(8, 3), (4, 1), (2, 7)]
    assert (8, 3) in places and (8, 5) in places
    for width, off in places:
        f = fields(vals, off, width)
        mid = int(np.sort(f)[n // 2])
        below, equal, above = int((f < mid).sum()), int((f == mid).sum()), int((f > mid).sum())
        assert equal >= 1 and below + equal + above == n
        # the field equal to the operand
        assert count(LT, off, width, mid) == below and count(LE, off, width, mid) == below + equal
        assert count(GT, off, width, mid) == above and count(GE, off, width, mid) == above + equal
        assert count(EQ, off, width, mid) == equal and count(NE, off, width, mid) == n - equal
        ones = (1 << (8 * width)) - 1
        if width < 8:  # an operand one bit wider than the field
            assert count(EQ, off, width, ones + 1) == 0 and count(LT, off, width, ones + 1) == n
            assert count(GE, off, width, ones + 1) == 0 and count(ANYBITS, off, width, ones + 1) == 0
        assert count(EQ, off, width, ones) >= 1  # (vals[1])
        top = 1 << (8 * width - 1)
        nbit = int(((f >> np.uint64(8 * width - 1)) & np.uint64(1)).sum())
        assert 1 <= nbit < n
        assert count(ANYBITS, off, width, top) == nbit and count(NOBITS, off, width, top) == n - nbit
        zeros = int((f == 0).sum())
        assert zeros >= 1  # (vals[0])
        assert count(ANYBITS, off, width, M64) == n - zeros and count(NOBITS, off, width, M64) == zeros
        assert count(ANYBITS, off, width, ones) == n - zeros
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 5. the empty key
def run_empty_key(lib, oracle_lib, dev, vs: int = 8, host_form: bool = False) -> None:
    """key_size 0: the one record is the one past the table (index cap)."""
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 0, vs, MC.HASH_MAX))
    snap = Snapshot(vm, ref, m, dev)
    assert len(check_scan(lib, vm, snap, m, dev, None, host_form=host_form)[0]) == 0  # an empty map
    val = (np.arange(vs, dtype=np.uint32) % 251 + 1).astype(np.uint8)[None, :]
    some, d_v = dev(np.zeros(64, dtype=np.uint8)), dev(val)
    settle(d_v)
    fn = lib.map_update_batch_device if on_dev(some) else lib.map_update_batch_staged
    assert fn(vm.h, m, addr(some), addr(d_v), 1, *([None] if on_dev(some) else [])) == 0, lib.last_error(vm.h)
    ref.map_update(m, b"", val.tobytes())
    snap = Snapshot(vm, ref, m, dev)
    assert list(snap.slots) == [MC.hash_geometry(vm, m)[0]]
    ek, ev, _ = check_scan(lib, vm, snap, m, dev, None, host_form=host_form)
    assert len(ek) == 1 and np.array_equal(ev, val)
    assert len(check_scan(lib, vm, snap, m, dev, MapFilter(EQ, 0, 1, 1), host_form=host_form)[0]) == 1
    assert len(check_scan(lib, vm, snap, m, dev, MapFilter(NE, 0, 1, 1), host_form=host_form)[0]) == 0
    ek, r = check_expire(lib, vm, ref, m, dev, MapFilter(GE, vs - 1, 1, 1), host_form=host_form)
    assert r == 1
    snap = Snapshot(vm, ref, m, dev)
    assert len(check_scan(lib, vm, snap, m, dev, None, host_form=host_form)[0]) == 0 and ref.map_lookup(m, b"") is None
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 6. nil-backed values
def run_vlen0(lib, oracle_lib, dev) -> None:
    """The setup of mapops_cases.run_vlen0: three of the four keys of a HASH map are left nil-backed
    (XE_SLOT_VLEN0: the stored bytes are an earlier value, the entry reads as zeros)."""
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
    marked = (w0 & np.uint64(MC.SLOT_VLEN0)) != 0
    assert int(marked.sum()) == 3, "the batch left no nil-backed records on the device"
    snap = Snapshot(vm, ref, m, dev)
    ek, ev, _ = check_scan(lib, vm, snap, m, dev, MapFilter(EQ, 0, 8, 0))
    assert sorted(int(k.view(np.uint32)[0]) for k in ek) == nil and not ev.any()
    ek, ev, _ = check_scan(lib, vm, snap, m, dev, MapFilter(NE, 0, 8, 0))
    assert len(ek) == 1 and int(ek[0].view(np.uint32)[0]) not in nil and ev.any()
    assert len(check_scan(lib, vm, snap, m, dev, None)[0]) == 4
    check_expire(lib, vm, ref, m, dev, MapFilter(EQ, 0, 8, 0), cap=2)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 7. alignment
def run_alignment(lib, oracle_lib, dev, ks: int, vs: int) -> None:
    """The outputs 0, 1, 4 and 8 bytes past a 16-byte boundary inside GUARD buffers (mo_move's unit: 16, 8
    or 4 bytes or single bytes, by how the record / the value and the output are aligned to each other)."""
    rng = np.random.default_rng(7000 + 10 * ks + vs)
    n = 130
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 2 * n))
    fill_hash(vm, ref, m, dev, rng, ks, vs, n)
    snap = Snapshot(vm, ref, m, dev)
    assert len(snap.keys) == n - (n + 2) // 3
    for koff in ALIGN_OFFSETS:
        for voff in ALIGN_OFFSETS:
            if koff != voff and (koff, voff) not in ((8, 1), (1, 8)):
                continue
            check_scan(lib, vm, snap, m, dev, None, koff=koff, voff=voff)
            check_scan(lib, vm, snap, m, dev, MapFilter(ANYBITS, 0, 1, 1), cap=7, koff=koff, voff=voff)
    check_expire(lib, vm, ref, m, dev, MapFilter(ANYBITS, 0, 1, 1), koff=1, voff=4)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 8. expire, then reuse
def run_expire_reuse(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(88)
    ks, vs = 16, 40
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, MC.HASH_MAX, delete_third=False)  # full
    vals[:, 0] = np.arange(MC.HASH_MAX) % 2  # half of them marked
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, m, keys, vals)
    before = Snapshot(vm, ref, m, dev)
    assert len(before.keys) == MC.HASH_MAX
    ek, r = check_expire(lib, vm, ref, m, dev, MapFilter(EQ, 0, 1, 1), host_visit=False)
    assert r == MC.HASH_MAX // 2
    img = state_image(vm, m, dev)
    assert int(((image_records(vm, m, img)[0] & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == before.tombs + r
    nv = rng.integers(0, 256, size=(r, vs), dtype=np.uint8)
    vm.map_update_batch_device(m, dev(np.ascontiguousarray(ek)), dev(nv))  # the records are taken again
    MC.ref_update(ref, m, ek, nv)
    img = same_image_map(vm, ref, m, dev, "expired keys installed again")
    w0 = image_records(vm, m, img)[0]
    assert int(((w0 & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == before.tombs
    after = Snapshot(vm, ref, m, dev)
    assert np.array_equal(after.slots, before.slots), "a key that came back did not take its old record"
    assert vm.map_count(m) == ref.map_count(m) == MC.HASH_MAX
    same_map(vm, ref, m, "expired keys installed again")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 9. under traffic
def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    r = Runner(vm, dev, use_async)
    # 32 flows: 24 that the batches carry (every one of them is hit) and 8 that no packet belongs to
    keys, vals = MC.flow_entries(list(range(24)) + [(1 << 41) + i for i in range(8)])
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    MC.ref_update(ref, rm, keys, vals)

    def ref_run(start: int) -> np.ndarray:
        umem, descs = MC.W.build_batch("c3learn", start, MC.FLOW_PACKETS)
        return ref.run_batch(umem, descs).verdicts

    idle = MapFilter(EQ, 8, 8, 0)  # flows never hit
    v0 = r.run(0)
    w0 = ref_run(0)
    # no xe_sync in between: the expire completes the pipeline itself. (An image taken here would complete
    # it first, so this call's answer is compared as a set; the order is checked by the scan below.)
    k, v, matched, _ = call(lib, vm, m, dev, idle, MC.FLOW_MAX, MC.FLOW_MAX, expire=True)
    assert np.array_equal(to_np(v0), w0)
    rk, rv = ref.map_dump(rm)
    sel = selects(rv, idle)
    assert int(sel.sum()) == 8 < len(rk)  # the eight flows without packets; learned flows start with one hit
    assert matched == int(sel.sum())
    gk, gv = MC.by_key(k, v)
    wk, wv = MC.by_key(rk[sel], rv[sel])
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), "the expired entries are not the oracle's idle flows"
    MC.ref_delete(ref, rm, rk[sel])
    v1 = r.run(MC.FLOW_PACKETS)
    w1 = ref_run(MC.FLOW_PACKETS)
    snap = Snapshot(vm, ref, m, dev)  # (completes the pipeline; compares the image with the oracle)
    assert np.array_equal(to_np(v1), w1)
    ek, _, _ = check_scan(lib, vm, snap, m, dev, None)
    assert len(ek) == ref.map_count(rm)
    check_scan(lib, vm, snap, m, dev, idle)
    same_map(vm, ref, m, "after two batches and an expire")
    # a host write, then a device scan: the map is uploaded first
    nk, _ = MC.flow_entries([1 << 40])
    vm.map_update(m, nk[0].tobytes(), b"\x42" * 16)
    ref.map_update(rm, nk[0].tobytes(), b"\x42" * 16)
    up, _ = vm.map_traffic(m)
    got = raw_call(lib, vm, m, MapFilter(EQ, 0, 8, 0x4242424242424242), 0, 0, 0, True, False)
    assert got == (0, 1) and vm.map_traffic(m)[0] == up + 1
    snap = Snapshot(vm, ref, m, dev)
    ek, _, _ = check_scan(lib, vm, snap, m, dev, MapFilter(EQ, 0, 8, 0x4242424242424242))
    assert len(ek) == 1 and np.array_equal(ek[0], nk[0])
    v2 = r.run(2 * MC.FLOW_PACKETS)
    w2 = ref_run(2 * MC.FLOW_PACKETS)
    same_map(vm, ref, m, "after three batches")
    assert np.array_equal(to_np(v2), w2)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 10. no whole-map traffic
def run_traffic(lib, dev) -> None:
    vm, m = flow_vm(lib)
    r = Runner(vm, dev, False)
    keys, vals = MC.flow_entries(list(range(56)) + [(1 << 41) + i for i in range(8)])  # eight flows without packets
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    r.run(0)  # the map is now newer on the device
    up, down = vm.map_traffic(m)
    for flt in (None, MapFilter(EQ, 8, 8, 0), MapFilter(NE, 8, 8, 0)):
        k, v, matched, _ = call(lib, vm, m, dev, flt, MC.FLOW_MAX, MC.FLOW_MAX)
        assert matched >= 1
    k, v, matched, _ = call(lib, vm, m, dev, MapFilter(EQ, 8, 8, 0), 5, 8, expire=True)
    assert matched == 8 and len(k) == 5
    # the delta base went to zero with the values: xe_map_delta (values - base, since the batch) reports
    # nothing on the expired records, whose base held the installed flow ids
    out = dev(np.full(vm.map_values_bytes(m), GUARD, np.uint8))
    settle(out)
    vm.map_delta(m, addr(out), lane=8)
    delta = to_np(out).reshape(-1, 16)
    w0, ikeys, _, _ = image_records(vm, m, state_image(vm, m, dev))
    for key in k:
        slot = np.nonzero((ikeys == key).all(axis=1) & (w0 == np.uint64(MC.SLOT_TOMB)))[0]
        assert len(slot) == 1 and key.any() and not delta[slot[0]].any(), "an expire left the delta base behind"
    assert delta.any(), "the batch's adds are not in the delta"
    assert vm.map_traffic(m) == (up, down), "a scan or an expire moved the whole map"
    r.run(MC.FLOW_PACKETS)  # a batch after the device expire: nothing to upload
    assert vm.map_traffic(m) == (up, down)
    vm.map_lookup(m, keys[0].tobytes())
    assert vm.map_traffic(m) == (up, down + 1), "the counter does not count the single-key path's download"
    vm.close()


# ---------------------------------------------------------------- 11. epoch
def run_epoch(lib, dev) -> None:
    vm, m = flow_vm(lib)
    keys, vals = MC.flow_entries(range(8))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    vm.epoch_begin()
    k, v, matched, _ = call(lib, vm, m, dev, None, 8, 8)
    assert matched == 8 and np.array_equal(MC.by_key(k, v)[1], MC.by_key(keys, vals)[1])
    for device_form in (True, False):
        rc, _ = raw_call(lib, vm, m, None, 0, 0, 8, device_form, True)
        assert rc == MC.ERR_INVAL
    assert raw_call(lib, vm, m, None, 0, 0, 0, True, False) == (0, 8)
    vm.epoch_end()
    assert raw_call(lib, vm, m, None, 0, 0, 3, True, True) == (0, 8)  # silently: no output buffers
    assert vm.map_count(m) == 5
    vm.close()


# ---------------------------------------------------------------- 12. limits
def run_limits(lib, oracle_lib, dev) -> None:
    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        d = MapDef(t, 4, 8, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 8, 16)
        m = vm.add_map(d)
        k, v = np.zeros((2, 4), np.uint8), np.zeros((2, 8), np.uint8)
        for device_form in (True, False):
            for expire in (False, True):
                rc, _ = raw_call(lib, vm, m, None, k.ctypes.data, v.ctypes.data, 2, device_form, expire)
                assert rc == MC.ERR_UNSUPPORTED
                assert b"ARRAY and HASH" in lib.last_error(vm.h)
        vm.close()

    rng = np.random.default_rng(12)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 8, 10))
    for device_form in (True, False):
        assert raw_call(lib, vm, m, None, 0, 0, 2, device_form, True)[0] == MC.ERR_INVAL  # as xe_map_delete
    assert raw_call(lib, vm, m, None, 0, 0, 2, True, False) == (0, 10)
    vm.close()
    ref.close()

    vs = 13
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, vs, MC.HASH_MAX))
    fill_hash(vm, ref, m, dev, rng, 8, vs, 30)
    before = state_image(vm, m, dev)
    bad = [N.MapFilter(9, 0, 1, 0, 0), N.MapFilter(0xffffffff, 0, 1, 0, 0),     # an unknown op
           N.MapFilter(EQ, 0, 1, 1, 0), N.MapFilter(ALL, 0, 1, 7, 0),            # pad
           N.MapFilter(EQ, 0, 0, 0, 0), N.MapFilter(EQ, 0, 3, 0, 0), N.MapFilter(EQ, 0, 16, 0, 0),  # width
           N.MapFilter(EQ, vs, 1, 0, 0), N.MapFilter(EQ, vs - 7, 8, 0, 0), N.MapFilter(EQ, 0xffffffff, 8, 0, 0),
           N.MapFilter(EQ, 0xfffffffc, 4, 0, 0)]                                 # a field outside the value
    for f in bad:
        for device_form in (True, False):
            for expire in (False, True):
                rc, n = raw_call(lib, vm, m, f, 0, 0, 5, device_form, expire)
                assert rc == MC.ERR_INVAL, (f.op, f.offset, f.width, f.pad)
    ok = N.MapFilter(EQ, vs - 8, 8, 0, 0)
    for device_form in (True, False):
        for expire in (False, True):
            assert raw_call(lib, vm, m, ok, 0, 0, 5, device_form, expire, matched=False)[0] == MC.ERR_INVAL  # a NULL matched
            assert raw_call(lib, vm, 99, ok, 0, 0, 5, device_form, expire)[0] == MC.ERR_INVAL  # a bad map index
    assert raw_call(lib, vm, m, N.MapFilter(ALL, 1000, 77, 0, 5), 0, 0, 0, True, False) == (0, 20)  # ALL ignores the field
    assert np.array_equal(before, state_image(vm, m, dev)), "a refused call changed the map"
    same_map(vm, ref, m, "after the refused calls")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 13. determinism
def run_determinism(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(13)
    ks, vs, n = 24, 65, 3000
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 4096))
    fill_hash(vm, ref, m, dev, rng, ks, vs, n)
    flt = MapFilter(GT, 3, 4, 1 << 30)
    first = call(lib, vm, m, dev, flt, n, n, koff=4, voff=1)
    second = call(lib, vm, m, dev, flt, n, n, koff=4, voff=1)
    live = n - (n + 2) // 3
    assert first[2] == second[2] and 0.5 * live < first[2] < live
    assert np.array_equal(first[3][0], second[3][0]) and np.array_equal(first[3][1], second[3][1])
    snap = Snapshot(vm, ref, m, dev)
    ek, ev = snap.expect(flt)
    assert np.array_equal(first[0], ek) and np.array_equal(first[1], ev)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- the Python interface
def run_python_api(lib, oracle_lib, dev, on_device: bool) -> None:
    rng = np.random.default_rng(14)
    ks, vs = 8, 24
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    fill_hash(vm, ref, m, dev, rng, ks, vs, 40)
    snap = Snapshot(vm, ref, m, dev)
    flt = MapFilter(ANYBITS, 2, 1, 1)
    ek, ev = snap.expect(flt)
    assert 5 <= len(ek) < len(snap.keys)
    k, v, matched = vm.map_scan(m, flt, on_device=on_device)  # cap None: count first, then fetch all
    assert on_dev(k) == on_device and matched == len(ek)
    assert np.array_equal(to_np(k), ek) and np.array_equal(to_np(v), ev)
    k, v, matched = vm.map_scan(m, cap=3, on_device=on_device)
    assert matched == len(snap.keys) and np.array_equal(to_np(k), snap.keys[:3]) and np.array_equal(to_np(v), snap.vals[:3])
    k, v, matched = vm.map_expire(m, flt, cap=4, on_device=on_device)
    assert matched == len(ek) and np.array_equal(to_np(k), ek[:4]) and np.array_equal(to_np(v), ev[:4])
    MC.ref_delete(ref, m, ek[:4])
    k, v, matched = vm.map_expire(m, flt, on_device=on_device)
    assert matched == len(ek) - 4 and np.array_equal(to_np(k), ek[4:])
    MC.ref_delete(ref, m, ek[4:])
    same_image_map(vm, ref, m, dev, "after map_expire")
    same_map(vm, ref, m, "after map_expire")
    # an ARRAY map: u32 indices
    am = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 10))
    vm.map_update(am, (7).to_bytes(4, "little"), b"\x05" * 8)
    k, v, matched = vm.map_scan(am, MapFilter(EQ, 0, 8, 0x0505050505050505), on_device=on_device)
    assert matched == 1 and to_np(k).view(np.uint32).tolist() == [[7]] and to_np(v).tolist() == [[5] * 8]
    vm.close()
    ref.close()
