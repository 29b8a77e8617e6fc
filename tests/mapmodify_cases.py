"""Shared cases of the device-side in-place edit of map value fields (xe_map_modify_device /
xe_map_modify_batch_device and their host-pointer forms): tests/test_mapmodify.py runs them on the host
simulation, tests/test_mapmodify_gpu.py on the product library.

No expected value comes from the code under test:
  * the ARITHMETIC is `model`, a restatement of the eleven ops over Python's unbounded integers, itself pinned
    by a table of hand-written vectors (VECTOR_TABLE) before anything else;
  * the STATE comes from a twin VM of the same library, built identically, that receives map_scan -> the
    model's edits (edit_rows) -> map_update_batch_device of the first r entries, the device round trip the
    call replaces: the exported state images must be equal bit for bit, and so must a full scan and the
    xe_map_delta of both (lane 1: every byte of the value region against the delta base); the modified
    entries show no delta. An oracle VM (oracle/liboracle.so) gets the same edited values through its
    single-key map_update and is compared through the image, and through the dump after a host visit;
  * what a call REPORTS is the first r matches of mapscan_cases.Snapshot, taken before the call.

`dev` turns a numpy array into what a call is given for device memory: the array itself on the host
simulation, a CUDA tensor on the product. Sizes: a tile is 256 slots; the value sub-groups (xe_mo_lanes) cut
at 16, 64 and 1,024 bytes; the single pass of the silent uncapped walk serves values up to kMmTileMax = 64
bytes, so both walks meet every size class through the silent and the reporting form."""
from __future__ import annotations

import ctypes as C

import numpy as np

import mapops_cases as MC
import mapscan_cases as SC
from gobpfld_amd import _native as N
from gobpfld_amd import workloads as W
from gobpfld_amd.asm import JEQ, JGT, JNE, XDP_DROP, XDP_PASS, XDP_REDIRECT, Asm
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, VM, MapDef,
                                  MapEdit, MapFilter, Settings)
from mapops_cases import GUARD, addr, guards_intact, image_records, on_dev, place, same_image_map, same_map, settle, state_image, to_np
from mapscan_cases import TILE, Snapshot, fill_hash, keys_for_slots, selects

SET, ADD, SUB, ADD_SAT, SUB_SAT, AND, OR, XOR, MIN, MAX, SHR = range(11)  # include/xdpemu.h XE_MM_*
OPS = (SET, ADD, SUB, ADD_SAT, SUB_SAT, AND, OR, XOR, MIN, MAX, SHR)
MAX_EDITS = 8
M64 = (1 << 64) - 1
WIDTHS = (1, 2, 4, 8)

MATRIX_VALUE_SIZES = (1, 8, 16, 17, 64, 65, 1024, 1025)
MATRIX_PAIRS = tuple([(ks, vs) for vs in MATRIX_VALUE_SIZES for ks in (8, 24)] + [(0, 24), (13, 24), (56, 24)])
ARRAY_VALUE_SIZES = (1, 24, 65, 1025)
ARRAY_ENTRIES = (1, 100, 4099)  # below a wave; below a tile; 17 tiles, the last one partial
SLOT_CASES = ((8, 16, 6), (128, TILE, 100), (256, 2 * TILE, 200))  # (max_entries, slots, live keys)
KEYED_COUNTS = (1, 255, 256, 257, 65537)
KEYED_VALUE_SIZES = (8, 24, 100, 1025)  # one per xe_mo_lanes class


# ---------------------------------------------------------------- the eleven ops, restated
def model(op: int, width: int, field: int, operand: int) -> int:
    """The new field, over unbounded integers (0 <= field < 2^(8 width), 0 <= operand < 2^64)."""
    top = (1 << (8 * width)) - 1
    if op == SET:
        return operand % (top + 1)
    if op == ADD:
        return (field + operand) % (top + 1)
    if op == SUB:
        return (field - operand) % (top + 1)
    if op == ADD_SAT:
        return min(field + operand, top)
    if op == SUB_SAT:
        return max(field - operand, 0)
    if op == AND:
        return field & operand
    if op == OR:
        return (field | operand) % (top + 1)
    if op == XOR:
        return (field ^ operand) % (top + 1)
    if op == MIN:
        return min(field, operand)
    if op == MAX:
        return min(max(field, operand), top)
    if op == SHR:
        return field >> operand if operand < 8 * width else 0
    raise ValueError(op)


# (op, width, field, operand, result), worked out by hand
VECTOR_TABLE = (
    # ADD wraps at width 1 and at width 8
    (ADD, 1, 0xff, 1, 0x00), (ADD, 1, 0xf0, 0x20, 0x10), (ADD, 1, 5, 0x1fe, 3), (ADD, 8, M64, 1, 0), (ADD, 8, M64, M64, M64 - 1),
    (ADD, 2, 0xfffe, 3, 1), (ADD, 4, 0xffffffff, 0xffffffff, 0xfffffffe), (ADD, 8, 1 << 63, 1 << 63, 0),
    # ADD_SAT reaching and passing the maximum
    (ADD_SAT, 1, 0xf0, 0x0f, 0xff), (ADD_SAT, 1, 0xf0, 0x10, 0xff), (ADD_SAT, 1, 0, 0x100, 0xff), (ADD_SAT, 2, 0xfff0, 0x0e, 0xfffe),
    (ADD_SAT, 2, 1, M64, 0xffff), (ADD_SAT, 4, 0xfffffffe, 1, 0xffffffff), (ADD_SAT, 4, 0xfffffffe, 2, 0xffffffff),
    (ADD_SAT, 8, M64 - 1, 1, M64), (ADD_SAT, 8, M64 - 1, 2, M64), (ADD_SAT, 8, 1 << 63, 1 << 63, M64), (ADD_SAT, 8, 3, 4, 7),
    # SUB_SAT at and below 0
    (SUB_SAT, 1, 5, 5, 0), (SUB_SAT, 1, 5, 6, 0), (SUB_SAT, 1, 5, 4, 1), (SUB_SAT, 1, 0xff, 0x1ff, 0), (SUB_SAT, 2, 0x100, 0xff, 1),
    (SUB_SAT, 4, 0, 1, 0), (SUB_SAT, 8, 1, M64, 0), (SUB_SAT, 8, M64, M64 - 1, 1), (SUB_SAT, 2, 0xffff, 1 << 16, 0),
    # SUB wraps
    (SUB, 1, 0, 1, 0xff), (SUB, 2, 1, 3, 0xfffe), (SUB, 4, 0, 1, 0xffffffff), (SUB, 8, 0, 1, M64), (SUB, 1, 0x10, 0x101, 0x0f),
    # SHR by 0, by 8 width - 1, by 8 width and by 200
    (SHR, 1, 0x80, 0, 0x80), (SHR, 1, 0x80, 7, 1), (SHR, 1, 0xff, 8, 0), (SHR, 1, 0xff, 200, 0),
    (SHR, 2, 0x8001, 0, 0x8001), (SHR, 2, 0x8001, 15, 1), (SHR, 2, 0xffff, 16, 0), (SHR, 2, 0xffff, 200, 0),
    (SHR, 4, 0x80000000, 31, 1), (SHR, 4, 0xffffffff, 32, 0), (SHR, 4, 0xffffffff, 200, 0), (SHR, 4, 0xf0, 4, 0x0f),
    (SHR, 8, 1 << 63, 63, 1), (SHR, 8, M64, 64, 0), (SHR, 8, M64, 200, 0), (SHR, 8, M64, 0, M64), (SHR, 8, M64, 1 << 32, 0),
    # MIN and MAX with an operand wider than the field
    (MIN, 1, 0x7f, 0x100, 0x7f), (MIN, 1, 0x7f, 0x10, 0x10), (MIN, 2, 0xffff, 1 << 40, 0xffff), (MIN, 4, 7, M64, 7), (MIN, 8, M64, 5, 5),
    (MAX, 1, 0x7f, 0x100, 0xff), (MAX, 1, 0x7f, 0x80, 0x80), (MAX, 2, 3, 1 << 40, 0xffff), (MAX, 4, 7, M64, 0xffffffff), (MAX, 8, 5, M64, M64),
    (MAX, 8, 9, 4, 9), (MAX, 2, 0x1234, 0x1233, 0x1234),
    # SET with a wide operand
    (SET, 1, 0x55, 0x1234, 0x34), (SET, 2, 0, 0x12345678, 0x5678), (SET, 4, 7, 0x1122334455667788, 0x55667788), (SET, 8, 1, M64, M64),
    # the bit ops
    (AND, 1, 0xf3, 0x10f, 0x03), (AND, 2, 0xffff, 0xff00ff00, 0xff00), (AND, 4, 0x12345678, 0, 0), (AND, 8, M64, 1 << 63, 1 << 63),
    (OR, 1, 0x01, 0x180, 0x81), (OR, 2, 0x0f00, 0x00f0, 0x0ff0), (OR, 4, 0, M64, 0xffffffff), (OR, 8, 1, 1 << 63, (1 << 63) | 1),
    (XOR, 1, 0xff, 0x10f, 0xf0), (XOR, 2, 0xaaaa, 0xffff, 0x5555), (XOR, 4, 1, 1, 0), (XOR, 8, M64, M64, 0),
)


def check_vector_table() -> None:
    seen = set()
    for op, width, field, operand, want in VECTOR_TABLE:
        assert 0 <= field < (1 << (8 * width)) and 0 <= operand <= M64
        assert model(op, width, field, operand) == want, (op, width, hex(field), hex(operand))
        seen.add((op, width))
    assert seen == {(op, w) for op in OPS for w in WIDTHS}, "every op at every width at least once"


def run_vectors(lib, dev) -> None:
    """The table through the library: one entry per vector in an ARRAY map, the field at byte 3 of a 13-byte
    value (aligned for no width), one keyed call per vector."""
    check_vector_table()
    vs, off = 13, 3
    vm = VM(Settings(engine=1), lib=lib)
    m = vm.add_map(MapDef(MAP_ARRAY, 4, vs, len(VECTOR_TABLE)))
    idx = np.arange(len(VECTOR_TABLE), dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vals = np.full((len(VECTOR_TABLE), vs), 0xC3, np.uint8)
    for i, (_, width, field, _, _) in enumerate(VECTOR_TABLE):
        vals[i, off:off + width] = np.frombuffer(field.to_bytes(width, "little"), np.uint8)
    vm.map_update_batch_device(m, dev(idx), dev(vals))
    want = vals.copy()
    for i, (op, width, _, operand, result) in enumerate(VECTOR_TABLE):
        old, found = vm.map_modify_batch(m, dev(idx[i:i + 1].copy()), [MapEdit(op, off, width, operand)])
        assert list(to_np(found)) == [1] and np.array_equal(to_np(old)[0], vals[i])
        want[i, off:off + width] = np.frombuffer(result.to_bytes(width, "little"), np.uint8)
    got, found = vm.map_lookup_batch(m, dev(idx))
    bad = np.nonzero((to_np(got) != want).any(axis=1))[0]
    assert not len(bad), [VECTOR_TABLE[i] for i in bad[:5]]
    vm.close()


def edit_rows(vals: np.ndarray, edits) -> np.ndarray:
    """The edit list applied to every row, by the model."""
    out = np.array(vals, dtype=np.uint8, copy=True)
    for row in out:
        for e in edits:
            w = e.width
            f = int.from_bytes(row[e.offset:e.offset + w].tobytes(), "little")
            o = int.from_bytes(row[e.operand:e.operand + w].tobytes(), "little") if e.operand_field else e.operand
            row[e.offset:e.offset + w] = np.frombuffer(model(e.op, w, f, o).to_bytes(w, "little"), np.uint8)
    return out


# ---------------------------------------------------------------- calls by address
def c_edits(edits):
    arr = (N.MapEdit * max(len(edits), 1))()
    for i, e in enumerate(edits):
        arr[i] = e if isinstance(e, N.MapEdit) else N.MapEdit(e.op, e.offset, e.width, 1 if e.operand_field else 0, e.operand)
    return arr


def c_filter(flt):
    if flt is None:
        return None
    return flt if isinstance(flt, N.MapFilter) else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand)


def raw_modify(lib, vm: VM, m: int, flt, edits, kptr, vptr, cap: int, device_form: bool, matched=True, n_edits=None, null_edits=False):
    """One walk call by address. Returns (rc, matched)."""
    cf, ce = c_filter(flt), c_edits(edits)
    n = C.c_uint64(0xDEADBEEF)
    head = (vm.h, m, None if cf is None else C.byref(cf), None if null_edits else ce, len(edits) if n_edits is None else n_edits,
            kptr or None, vptr or None, cap, C.byref(n) if matched else None)
    rc = lib.map_modify_device(*head, None) if device_form else lib.map_modify(*head)
    return rc, n.value


def raw_modify_batch(lib, vm: VM, m: int, kptr, count: int, edits, vptr, fptr, device_form: bool, n_edits=None, null_edits=False):
    ce = c_edits(edits)
    head = (vm.h, m, kptr or None, count, None if null_edits else ce, len(edits) if n_edits is None else n_edits, vptr or None,
            fptr or None)
    return lib.map_modify_batch_device(*head, None) if device_form else lib.map_modify_batch(*head)


def trio(lib, oracle_lib, mdef: MapDef):
    """The VM under test, its twin of the same library, the oracle, the map's index in all three."""
    vm, twin, ref = VM(Settings(engine=1), lib=lib), VM(Settings(engine=1), lib=lib), VM(Settings(engine=1), lib=oracle_lib)
    m = vm.add_map(mdef)
    assert twin.add_map(mdef) == m and ref.add_map(mdef) == m
    return vm, twin, ref, m


def close(*vms) -> None:
    for v in vms:
        v.close()


def clone_state(vm: VM, m: int, dev, *others: VM) -> None:
    """The VM's exported state imported into the other VMs: the same records in the same slots. (Keys that a
    batch inserts in one launch race for the free records of a shared probe chain, so two VMs given the same
    calls need not end with the same layout.)"""
    img = dev(state_image(vm, m, dev))
    settle(img)
    for v in others:
        v.map_state_import(m, addr(img))


def fill3(vm, twin, ref, m, dev, rng, ks: int, vs: int, n: int, delete_third: bool = True):
    """mapscan_cases.fill_hash on the VM and the oracle; the twin gets the VM's state."""
    keys, vals = fill_hash(vm, ref, m, dev, rng, ks, vs, n, delete_third)
    clone_state(vm, m, dev, twin)
    return keys, vals


def update_by_address(lib, vm: VM, m: int, dev, keys: np.ndarray, vals: np.ndarray) -> None:
    """map_update_batch_device, also for the empty key (whose key array has no address of its own)."""
    if not len(vals):
        return
    if keys.shape[1]:
        return vm.map_update_batch_device(m, dev(np.ascontiguousarray(keys)), dev(np.ascontiguousarray(vals)))
    some, d_v = dev(np.zeros(64, dtype=np.uint8)), dev(np.ascontiguousarray(vals))
    settle(d_v)
    if on_dev(some):
        rc = lib.map_update_batch_device(vm.h, m, addr(some), addr(d_v), len(vals), None)
    else:
        rc = lib.map_update_batch_staged(vm.h, m, addr(some), addr(d_v), len(vals))
    assert rc == 0, lib.last_error(vm.h)


def delta_bytes(vm: VM, m: int, dev) -> np.ndarray:
    """xe_map_delta with one-byte lanes: value region minus delta base, byte by byte."""
    out = dev(np.full(vm.map_values_bytes(m), GUARD, np.uint8))
    settle(out)
    vm.map_delta(m, addr(out), lane=1)
    return to_np(out).copy()


def full_scan(lib, vm: VM, m: int, dev, room: int):
    k, v, matched, _ = SC.call(lib, vm, m, dev, None, room, room)
    assert matched == len(k)
    return k, v


def same_state(lib, vm: VM, twin: VM, m: int, dev, room: int, what: str, with_delta: bool = True):
    """Image, full scan and delta of the VM and of its twin. Returns (image, scan keys, scan values, delta)."""
    img, timg = state_image(vm, m, dev), state_image(twin, m, dev)
    assert np.array_equal(img, timg), f"{what}: the state image differs from the twin's (scan, edit, update)"
    k, v = full_scan(lib, vm, m, dev, room)
    tk, tv = full_scan(lib, twin, m, dev, room)
    assert np.array_equal(k, tk) and np.array_equal(v, tv), f"{what}: a full scan differs from the twin's"
    d = None
    if with_delta:
        d, td = delta_bytes(vm, m, dev), delta_bytes(twin, m, dev)
        assert np.array_equal(d, td), f"{what}: xe_map_delta differs from the twin's"
    return img, k, v, d


def check_modify(lib, vm, twin, ref, m, dev, edits, flt=None, cap=None, report: bool = True, host_form: bool = False, koff: int = 0,
                 voff: int = 0, want_keys: bool = True, want_vals: bool = True, host_visit: bool = False, with_delta: bool = True):
    """One walk call against the state before it. cap None: 2^64 - 1 (uncapped). report False: both output
    pointers NULL. Returns (expected keys, r)."""
    d = vm.map_defs[m]
    array = d.type == MAP_ARRAY
    ks, vs = (4 if array else d.key_size), d.value_size
    before = Snapshot(vm, ref, m, dev)
    ek, ev = before.expect(flt)
    cap = M64 if cap is None else cap
    r = min(cap, len(ek))
    what = f"modify {[(e.op, e.offset, e.width, e.operand, e.operand_field) for e in edits]} cap {cap} report {report}"
    # the call, into guard buffers of r + 3 entries
    mk = np.ascontiguousarray if host_form else dev
    kbuf, _ = place(mk, np.full((r + 3, ks), GUARD, np.uint8), koff)
    vbuf, _ = place(mk, np.full((r + 3, vs), GUARD, np.uint8), voff)
    settle(kbuf)
    settle(vbuf)
    want_keys, want_vals = want_keys and report, want_vals and report
    rc, matched = raw_modify(lib, vm, m, flt, edits, addr(kbuf) + koff if want_keys else 0, addr(vbuf) + voff if want_vals else 0, cap,
                             not host_form)
    assert rc == 0, lib.last_error(vm.h)
    assert matched == len(ek), f"{what}: matched {matched}, expected {len(ek)}"
    k = guards_intact(kbuf, koff, r * ks if want_keys else 0, what + ": keys")
    v = guards_intact(vbuf, voff, r * vs if want_vals else 0, what + ": values")
    if want_keys:
        assert np.array_equal(k.reshape(-1, ks) if ks else np.zeros((r, 0), np.uint8), ek[:r]), f"{what}: keys differ (or their order)"
    if want_vals:
        assert np.array_equal(v.reshape(-1, vs), ev[:r]), f"{what}: the values from before the edits are reported"
    # the twin: scan, the model's edits, update of the first r
    tk, tv, tm = twin.map_scan(m, flt)
    assert tm == len(ek) and np.array_equal(tk, ek) and np.array_equal(tv, ev), "the twin's scan is not the snapshot's"
    new = edit_rows(ev[:r], edits)
    update_by_address(lib, twin, m, dev, ek[:r], new)
    MC.ref_update(ref, m, ek[:r], new)
    room = d.max_entries if array else len(before.keys)
    img, sk, sv, delta = same_state(lib, vm, twin, m, dev, room, what, with_delta)
    # the scan against the model directly: the first r matches edited, every other entry as it was
    after = before.vals.copy()
    hit = np.nonzero(selects(before.vals, flt))[0][:r]
    after[hit] = new
    assert np.array_equal(sk, before.keys) and np.array_equal(sv, after), f"{what}: the entries after the call are not the model's"
    if with_delta:  # the modified entries show no delta: their whole value went to the delta base
        slots = hit if array else before.slots[hit]
        dv = delta[:(int(slots.max()) + 1) * vs].reshape(-1, vs) if len(slots) else np.zeros((0, vs), np.uint8)
        assert not dv[slots].any(), f"{what}: a modified entry shows up in xe_map_delta"
    if not array:
        w0 = image_records(vm, m, img)[0]
        assert (w0[before.slots[hit]] == np.uint64(MC.SLOT_FULL)).all(), f"{what}: a modified record is not plain FULL"
        assert int(((w0 & np.uint64(MC.SLOT_TOMB)) != 0).sum()) == before.tombs, f"{what}: the tombstones changed"
        same_image_map(vm, ref, m, dev, what)
    if host_visit:  # (both: a host visit rebuilds the table without its tombstones)
        same_map(vm, ref, m, what)
        same_map(twin, ref, m, what + " (twin)")
    return ek, r


def operand_for(op: int, width: int) -> int:
    """An operand that makes the op's special cases happen on random fields: wraps, saturations, a wide operand."""
    top = (1 << (8 * width)) - 1
    return {SET: 0x0123456789abcdef, ADD: 0xf1f2f3f4f5f6f7f8 & top | 1, SUB: (top >> 1) + 2, ADD_SAT: (top >> 1) + 1, SUB_SAT: (top >> 1) + 1,
            AND: 0x0ff00ff00ff00ff0, OR: 0x8000000000000001, XOR: M64, MIN: top >> 1, MAX: (top >> 1) + 1, SHR: 3}[op]


# ---------------------------------------------------------------- 1. matrices
def run_hash_matrix(lib, oracle_lib, dev, ks: int, vs: int, host_form: bool = False) -> None:
    """Every op at the widest field that fits, at the value's end, on the entries a filter selects: the silent
    uncapped form (the single pass up to 64-byte values) and the reporting form each."""
    if ks == 0:
        return run_empty_key(lib, oracle_lib, dev, vs, host_form)
    rng = np.random.default_rng(5000 * ks + vs)
    n = 300
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, 512))  # 1,024 slots: four tiles
    fill3(vm, twin, ref, m, dev, rng, ks, vs, n)
    width = SC.widest(vs)
    off = vs - width
    flt = MapFilter(SC.ANYBITS, 0, 1, 0x3)  # about three quarters, decided on the value from before the edit
    for i, op in enumerate(OPS):
        edit = [MapEdit(op, off, width, operand_for(op, width))]
        ek, r = check_modify(lib, vm, twin, ref, m, dev, edit, flt, report=False, host_form=host_form)
        assert r == len(ek) and (vs <= 8 or 100 <= r < 200)  # (up to 8 bytes the edited field covers the filter's byte)
        check_modify(lib, vm, twin, ref, m, dev, edit, flt, cap=512, report=True, host_form=host_form, host_visit=i == len(OPS) - 1)
    if vs >= 2 * width:  # the operand from the value's first field
        check_modify(lib, vm, twin, ref, m, dev, [MapEdit(ADD, off, width, 0, True)], None, report=False, host_form=host_form)
        check_modify(lib, vm, twin, ref, m, dev, [MapEdit(SUB_SAT, off, width, 0, True)], None, cap=77, host_form=host_form)
    close(vm, twin, ref)


def run_array_matrix(lib, oracle_lib, dev, vs: int, entries: int, host_form: bool = False) -> None:
    rng = np.random.default_rng(6000 * vs + entries)
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, entries))
    idx = np.ascontiguousarray(rng.permutation(entries)[: (entries + 1) // 2].astype(np.uint32)).view(np.uint8).reshape(-1, 4)
    vals = rng.integers(0, 256, size=(len(idx), vs), dtype=np.uint8)
    for v in (vm, twin):
        v.map_update_batch_device(m, dev(idx), dev(vals))
    MC.ref_update(ref, m, idx, vals)
    width = SC.widest(vs)
    off = vs - width
    for op in (ADD, SUB_SAT, XOR):
        edit = [MapEdit(op, off, width, operand_for(op, width))]
        ek, r = check_modify(lib, vm, twin, ref, m, dev, edit, None, report=False, host_form=host_form)  # every index is an entry
        assert r == entries
        check_modify(lib, vm, twin, ref, m, dev, edit, MapFilter(SC.NE, off, width, 0), cap=entries, host_form=host_form)
    check_modify(lib, vm, twin, ref, m, dev, [MapEdit(SET, 0, 1, 0x5a)], MapFilter(SC.ANYBITS, 0, 1, 1), cap=entries // 2 + 1,
                 want_vals=False, host_form=host_form, host_visit=True)
    close(vm, twin, ref)


def run_array_tile_plus_one(lib, oracle_lib, dev) -> None:
    """TILE + 1 indices, the only match in the last one: the second tile's only slot."""
    vs, entries = 8, TILE + 1
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_ARRAY, 4, vs, entries))
    idx = np.array([TILE], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vals = np.array([[3] * vs], dtype=np.uint8)
    for v in (vm, twin):
        v.map_update_batch_device(m, dev(idx), dev(vals))
    MC.ref_update(ref, m, idx, vals)
    for report in (False, True):
        ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(ADD, 0, 8, 1 << 56)], MapFilter(SC.EQ, 0, 1, 3), cap=entries, report=report)
        assert r == 1 and np.array_equal(ek, idx)
    ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(OR, 4, 4, 0x80)], MapFilter(SC.EQ, 0, 8, 0), report=False, host_visit=True)
    assert r == TILE
    close(vm, twin, ref)


# ---------------------------------------------------------------- 2. slot counts
def keys_at(cap: int, homes, n: int) -> np.ndarray:
    """n distinct 8-byte keys (counters): one with its home in each slot of `homes`, first, then the first
    counters that are none of them (keys_for_slots, for any slots)."""
    c = np.arange(1, 16 * max(cap, 1024) + 1, dtype=np.uint64)
    home = (SC.hash8(c) & np.uint64(0xffffffff)) & np.uint64(cap - 1)
    first = np.array([c[home == np.uint64(h)][0] for h in homes], dtype=np.uint64)
    rest = c[~np.isin(c, first)][: n - len(first)]
    return np.ascontiguousarray(np.concatenate([first, rest]).view(np.uint8).reshape(-1, 8))


def run_slot_counts(lib, oracle_lib, dev, max_entries: int, slots: int, live: int) -> None:
    """Matches in the first and the last slot of the table, and of a tile where the table has two."""
    rng = np.random.default_rng(slots + 1)
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, 8, 8, max_entries))
    assert MC.hash_geometry(vm, m)[0] == slots
    assert np.array_equal(keys_at(slots, (0, slots - 1), live), keys_for_slots(slots, live))
    homes = (0, slots - 1) + ((TILE - 1, TILE) if slots > TILE else ())
    keys = keys_at(slots, homes, live)
    vals = rng.integers(0, 256, size=(live, 8), dtype=np.uint8)
    vals[:, 7] = 0
    vals[:len(homes), 7] = 0xEE  # the marked entries: the ones in the edge slots
    vm.map_update_batch_device(m, dev(keys[:len(homes)].copy()), dev(vals[:len(homes)].copy()))  # first: they get their home slots
    vm.map_update_batch_device(m, dev(keys[len(homes):].copy()), dev(vals[len(homes):].copy()))
    clone_state(vm, m, dev, twin)
    MC.ref_update(ref, m, keys, vals)
    snap = Snapshot(vm, ref, m, dev)
    assert set(homes) <= set(snap.slots.tolist()) and snap.slots[0] == 0 and snap.slots[-1] == slots - 1
    edge = MapFilter(SC.EQ, 7, 1, 0xEE)
    for report in (False, True):
        ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(ADD, 0, 4, 0x01010101)], edge, cap=max_entries, report=report)
        assert r == len(homes) and sorted(map(bytes, ek)) == sorted(map(bytes, keys[:len(homes)]))
        ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(XOR, 0, 2, 0xffff)], None, report=report)
        assert r == live
        ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(SET, 0, 1, 9)], MapFilter(SC.EQ, 7, 1, 0x77), report=report)
        assert r == 0
    close(vm, twin, ref)


# ---------------------------------------------------------------- 3. fields and edit lists
def run_fields(lib, oracle_lib, dev, vs: int, host_form: bool = False) -> None:
    """Fields at offsets 0, 1, 3 and value_size - width for every width; values of 13 and 100 bytes put the map's
    own values at every alignment, and the outputs sit 0, 1, 4 and 8 bytes past a 16-byte boundary."""
    rng = np.random.default_rng(7700 + vs)
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, 8, vs, MC.HASH_MAX))
    fill3(vm, twin, ref, m, dev, rng, 8, vs, 48)
    places = [(w, off) for w in WIDTHS for off in dict.fromkeys((0, 1, 3, vs - w))]
    for i, (w, off) in enumerate(places):
        op = OPS[i % len(OPS)]
        offs = SC.ALIGN_OFFSETS[i % 4], SC.ALIGN_OFFSETS[(i // 4) % 4]
        check_modify(lib, vm, twin, ref, m, dev, [MapEdit(op, off, w, operand_for(op, w))], MapFilter(SC.ANYBITS, vs - 1, 1, 0x7),
                     cap=20, koff=offs[0], voff=offs[1], host_form=host_form)
        check_modify(lib, vm, twin, ref, m, dev, [MapEdit(ADD, off, w, 0x0101010101010101)], None, report=False)
    close(vm, twin, ref)


def run_edit_lists(lib, oracle_lib, dev, vs: int = 24, host_form: bool = False) -> None:
    rng = np.random.default_rng(7800 + vs)
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, 13, vs, MC.HASH_MAX))
    fill3(vm, twin, ref, m, dev, rng, 13, vs, 60)
    lists = {
        # overlapping fields: a later edit sees the earlier ones
        "overlap": [MapEdit(SET, 0, 8, 0x1111111111111111), MapEdit(ADD, 4, 8, 0xf0f0f0f0f0f0f0f0), MapEdit(SHR, 3, 4, 4),
                    MapEdit(XOR, 5, 2, 0xffff), MapEdit(SUB, 5, 1, 7)],
        # XE_MM_MAX_EDITS edits, one of every width twice
        "eight": [MapEdit(OPS[i], (3 * i) % (vs - 8), WIDTHS[i % 4], operand_for(OPS[i], WIDTHS[i % 4])) for i in range(MAX_EDITS)],
        # an operand field that an earlier edit wrote, and one that a later edit overwrites
        "operand written": [MapEdit(SET, 8, 4, 0x00c0ffee), MapEdit(ADD, 0, 4, 8, True), MapEdit(SET, 8, 4, 0), MapEdit(MAX, 16, 4, 8, True)],
        # the token bucket: tokens (u64 at 0) += rate (u32 at 8 ... as a u64 field at 8), capped at burst (u64 at 16)
        "token bucket": [MapEdit(ADD_SAT, 0, 8, 8, True), MapEdit(MIN, 0, 8, 16, True)],
        # the same op twice: ADD is applied twice
        "twice": [MapEdit(ADD, 1, 2, 0x7fff), MapEdit(ADD, 1, 2, 0x7fff)],
    }
    assert len(lists["eight"]) == MAX_EDITS
    for i, (name, edits) in enumerate(lists.items()):
        check_modify(lib, vm, twin, ref, m, dev, edits, MapFilter(SC.NOBITS, 2, 1, 0x4), report=False, host_form=host_form)
        check_modify(lib, vm, twin, ref, m, dev, edits, MapFilter(SC.NOBITS, 2, 1, 0x4), cap=64, voff=1, host_form=host_form,
                     host_visit=i == len(lists) - 1)
    close(vm, twin, ref)


def run_token_bucket(lib, oracle_lib, dev) -> None:
    """tokens = min(tokens + rate, burst) with rate and burst in the value, checked against plain arithmetic."""
    n = 100
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 24, n))
    rec = np.zeros(n, dtype=[("tokens", "<u8"), ("rate", "<u8"), ("burst", "<u8")])
    rec["tokens"], rec["rate"], rec["burst"] = np.arange(n) * 3, np.arange(n) % 7 + 1, 120 + np.arange(n) % 5
    rec["tokens"][5], rec["rate"][5], rec["burst"][5] = M64 - 1, 9, M64  # the sum saturates instead of wrapping past the burst
    idx = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vals = rec.view(np.uint8).reshape(n, 24)
    for v in (vm, twin):
        v.map_update_batch_device(m, dev(idx), dev(vals))
    MC.ref_update(ref, m, idx, vals)
    bucket = [MapEdit(ADD_SAT, 0, 8, 8, True), MapEdit(MIN, 0, 8, 16, True)]
    check_modify(lib, vm, twin, ref, m, dev, bucket, None, report=False)
    got = to_np(vm.map_lookup_batch(m, dev(idx))[0]).copy().view(rec.dtype).reshape(n)
    want = [min(min(int(t) + int(r), M64), int(b)) for t, r, b in zip(rec["tokens"], rec["rate"], rec["burst"])]
    assert got["tokens"].tolist() == want and want[5] == M64
    assert np.array_equal(got["rate"], rec["rate"]) and np.array_equal(got["burst"], rec["burst"])
    check_modify(lib, vm, twin, ref, m, dev, bucket, MapFilter(SC.LT, 0, 8, 121), cap=n, host_visit=True)
    close(vm, twin, ref)


# ---------------------------------------------------------------- 4. cap_entries
def run_caps(lib, oracle_lib, dev, report: bool, host_form: bool = False) -> None:
    """Only the first r matches change (check_modify: every other entry is the snapshot's), with and without
    outputs. A 24-byte value goes the general way when capped and the single pass when not."""
    ks, vs = 13, 24
    flt = MapFilter(SC.ANYBITS, 5, 2, 0x0101)
    rng = np.random.default_rng(44)
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    fill3(vm, twin, ref, m, dev, rng, ks, vs, 60)
    matched = len(Snapshot(vm, ref, m, dev).expect(flt)[0])
    assert 10 <= matched < 40
    for cap in (0, 1, matched - 1, matched, matched + 1, MC.HASH_MAX, M64):
        # (the edit keeps the filter's field: the same entries match every time)
        ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(ADD, 8, 8, 1), MapEdit(XOR, 0, 1, 0xff)], flt, cap=cap, report=report,
                             host_form=host_form)
        assert len(ek) == matched and r == min(cap, matched)
    close(vm, twin, ref)


# ---------------------------------------------------------------- 5. the empty key
def run_empty_key(lib, oracle_lib, dev, vs: int = 24, host_form: bool = False) -> None:
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, 0, vs, MC.HASH_MAX))
    edit = [MapEdit(ADD, vs - 8, 8, 0x0101010101010101)]
    for report in (False, True):  # an empty map
        assert check_modify(lib, vm, twin, ref, m, dev, edit, None, report=report, host_form=host_form)[1] == 0
    val = (np.arange(vs, dtype=np.uint32) % 251 + 1).astype(np.uint8)[None, :]
    for v in (vm, twin):
        update_by_address(lib, v, m, dev, np.zeros((1, 0), np.uint8), val)
    ref.map_update(m, b"", val.tobytes())
    assert list(Snapshot(vm, ref, m, dev).slots) == [MC.hash_geometry(vm, m)[0]]  # the record past the table
    for report in (False, True):
        assert check_modify(lib, vm, twin, ref, m, dev, edit, MapFilter(SC.EQ, 0, 1, 1), report=report, host_form=host_form)[1] == 1
        assert check_modify(lib, vm, twin, ref, m, dev, edit, MapFilter(SC.NE, 0, 1, 1), report=report, host_form=host_form)[1] == 0
    # keyed: three repetitions of the one key
    some = dev(np.zeros(64, dtype=np.uint8))
    d_v, d_f = dev(np.full((3, vs), GUARD, np.uint8)), dev(np.full(3, GUARD, np.uint8))
    settle(d_v)
    old = ref.map_lookup(m, b"")
    assert raw_modify_batch(lib, vm, m, addr(some), 3, [MapEdit(ADD, 0, 1, 1)], addr(d_v), addr(d_f), on_dev(some)) == 0
    assert list(to_np(d_f)) == [1, 1, 1] and all(v.tobytes() == old for v in to_np(d_v))
    new = edit_rows(np.frombuffer(old, np.uint8)[None, :], [MapEdit(ADD, 0, 1, 1)])
    update_by_address(lib, twin, m, dev, np.zeros((1, 0), np.uint8), new)
    ref.map_update(m, b"", new.tobytes())
    same_state(lib, vm, twin, m, dev, 1, "the empty key, keyed")
    same_image_map(vm, ref, m, dev, "the empty key, keyed")
    same_map(vm, ref, m, "the empty key")
    close(vm, twin, ref)


# ---------------------------------------------------------------- 6. nil-backed values
def run_vlen0(lib, oracle_lib, dev) -> None:
    """The setup of mapscan_cases.run_vlen0: a batch leaves three of the four keys of a HASH map nil-backed.
    Two of them are selected and become ordinary values (zeros plus the edits), the third stays nil-backed."""
    from parity import packets
    from test_lru_nil_value import _program
    umem, descs = packets(600, 64, seed=9)
    for d in descs:
        umem[int(d["addr"]) + 1] = 0
    for i in (150, 151, 400):
        umem[int(descs[i]["addr"]) + 1] = 1
    vms = []
    for lb in (lib, lib, oracle_lib):
        vm = VM(Settings(engine=1), lib=lb)
        m = vm.add_map(MapDef(MAP_HASH, 4, 8, 16))
        vm.set_entrypoint(vm.add_raw_program(_program()))
        vms.append((vm, vm.run_batch(umem.copy(), descs)))
    (vm, got), (twin, _), (ref, want) = vms
    assert np.array_equal(got.verdicts, want.verdicts)
    clone_state(vm, m, dev, vm, twin)  # (both: an import also sets the delta base)

    def marked() -> int:
        return int(((image_records(vm, m, state_image(vm, m, dev))[0] & np.uint64(MC.SLOT_VLEN0)) != 0).sum())

    assert marked() == 3, "the batch left no nil-backed records on the device"
    nil = MapFilter(SC.EQ, 0, 8, 0)
    edit = [MapEdit(OR, 0, 2, 0x0180), MapEdit(ADD, 1, 4, 0xffffffff)]
    ek, r = check_modify(lib, vm, twin, ref, m, dev, edit, nil, cap=2)  # (check_modify: the values reported are zeros)
    assert len(ek) == 3 and r == 2 and marked() == 1
    ek, r = check_modify(lib, vm, twin, ref, m, dev, edit, MapFilter(SC.NE, 0, 8, 0), report=False)  # the single pass; the nil one is not selected
    assert r == 3 and marked() == 1
    ek, r = check_modify(lib, vm, twin, ref, m, dev, [MapEdit(SET, 7, 1, 0x42)], nil, report=False, host_visit=True)  # the single pass on a nil value
    assert r == 1
    assert vm.map_lookup(m, ek[0].tobytes()) == bytes(7) + b"\x42"
    close(vm, twin, ref)


def run_vlen0_sizes(lib, oracle_lib, dev, vs: int) -> None:
    """Nil-backed values of every sub-group class: the VLEN0 bit is set on every fourth FULL record of an image,
    which is imported back (the stored bytes stay: an earlier value), and the oracle's values are zeroed."""
    rng = np.random.default_rng(6600 + vs)
    ks, n = 8, 60
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    fill3(vm, twin, ref, m, dev, rng, ks, vs, n)
    img = state_image(vm, m, dev)
    cap, rw, vals_alloc = MC.hash_geometry(vm, m)
    rec = img[vals_alloc:vals_alloc + (cap + 1) * rw * 8].view(np.uint64).reshape(cap + 1, rw)
    full = np.nonzero(rec[:, 0] & np.uint64(MC.SLOT_FULL))[0]
    keys = np.ascontiguousarray(rec[:, 1:]).view(np.uint8).reshape(cap + 1, (rw - 1) * 8)[:, :ks]
    nil = full[::4]
    rec[nil, 0] |= np.uint64(MC.SLOT_VLEN0)
    for v in (vm, twin):
        d_img = dev(img)
        settle(d_img)
        v.map_state_import(m, addr(d_img))
    MC.ref_update(ref, m, keys[nil], np.zeros((len(nil), vs), np.uint8))
    width = SC.widest(vs)
    edit = [MapEdit(OR, vs - width, width, 0x81), MapEdit(ADD, 0, 1, 3)]
    zero = MapFilter(SC.EQ, vs - 1, 1, 0)  # the nil-backed ones (and a random value in 256)
    ek, r = check_modify(lib, vm, twin, ref, m, dev, edit, zero, cap=len(nil) // 2)
    assert r == len(nil) // 2 and len(ek) >= len(nil)
    ek, r = check_modify(lib, vm, twin, ref, m, dev, edit, MapFilter(SC.ANYBITS, 0, 1, 1), report=False)  # nil ones read as 0: not selected
    w0 = image_records(vm, m, state_image(vm, m, dev))[0]
    assert int(((w0 & np.uint64(MC.SLOT_VLEN0)) != 0).sum()) == len(nil) - len(nil) // 2, "an unselected nil-backed record was touched"
    check_modify(lib, vm, twin, ref, m, dev, edit, zero, report=False, host_visit=True)
    close(vm, twin, ref)


# ---------------------------------------------------------------- 7. the keyed form
def check_modify_batch(lib, vm, twin, ref, m, dev, keys: np.ndarray, edits, host_form: bool = False, want_vals: bool = True,
                       want_found: bool = True, koff: int = 0, voff: int = 0) -> None:
    d = vm.map_defs[m]
    array = d.type == MAP_ARRAY
    ks, vs, n = (4 if array else d.key_size), d.value_size, len(keys)
    what = f"modify batch of {n}"
    wv, wf = MC.ref_lookup(ref, m, keys, vs)  # the oracle's single-key lookups: the same for every repetition of a key
    mk = np.ascontiguousarray if host_form else dev
    kbuf, kview = place(mk, keys, koff)
    vbuf, _ = place(mk, np.full((n, vs), GUARD, np.uint8), voff)
    fbuf, _ = place(mk, np.full(n, GUARD, np.uint8), koff)
    for b in (kbuf, vbuf, fbuf):
        settle(b)
    rc = raw_modify_batch(lib, vm, m, addr(kbuf) + koff, n, edits, addr(vbuf) + voff if want_vals else 0, addr(fbuf) + koff if want_found else 0,
                          not host_form)
    assert rc == 0, lib.last_error(vm.h)
    MC.unchanged(kbuf, koff, keys, what + ": keys")
    v = guards_intact(vbuf, voff, n * vs if want_vals else 0, what + ": values")
    f = guards_intact(fbuf, koff, n if want_found else 0, what + ": found")
    if want_found:
        assert np.array_equal(f, wf), f"{what}: found differs"
    if want_vals:
        assert np.array_equal(v.reshape(-1, vs), wv), f"{what}: the values from before the call differ (every repetition gets the same)"
    # each distinct present key once
    present = keys[wf != 0]
    uk, first = np.unique(present, axis=0, return_index=True)
    new = edit_rows(wv[wf != 0][first], edits)
    if len(uk):
        twin.map_update_batch_device(m, dev(np.ascontiguousarray(uk)), dev(new))
        MC.ref_update(ref, m, uk, new)
    room = d.max_entries if array else ref.map_count(m)
    img, _, _, delta = same_state(lib, vm, twin, m, dev, room, what)
    if not array:
        image_records(vm, m, img)  # (asserts that every last-writer word is zero again)
        same_image_map(vm, ref, m, dev, what)
    got, found = vm.map_lookup_batch(m, dev(np.ascontiguousarray(keys[:300])))
    assert np.array_equal(to_np(found), wf[:300])
    ev, _ = MC.ref_lookup(ref, m, keys[:300], vs)
    assert np.array_equal(to_np(got), ev), f"{what}: a key was not edited exactly once"


def run_keyed(lib, oracle_lib, dev, kind: int, vs: int, host_form: bool = False) -> None:
    """Present, absent and repeated keys in one batch; ADD by 1 shows "once per distinct key"."""
    rng = np.random.default_rng(9000 + vs + kind)
    array = kind == MAP_ARRAY
    ks = 4 if array else 13
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(kind, ks, vs, 100 if array else MC.HASH_MAX))
    if array:
        pool = np.arange(100, dtype=np.uint32).view(np.uint8).reshape(-1, 4)[rng.permutation(100)[:40]]
        absent = np.array([100, 107, 0xffffffff, 0x80000000], dtype=np.uint32).view(np.uint8).reshape(-1, 4)  # out of range
        vals = rng.integers(0, 256, size=(40, vs), dtype=np.uint8)
        for v in (vm, twin):
            v.map_update_batch_device(m, dev(np.ascontiguousarray(pool)), dev(vals))
        MC.ref_update(ref, m, pool, vals)
    else:
        keys, _ = fill3(vm, twin, ref, m, dev, rng, ks, vs, 60)
        live = np.ones(60, bool)
        live[::3] = False
        pool, absent = keys[live], np.concatenate([keys[~live][:4], MC.hash_pool(rng, ks, 4)])  # deleted keys and keys never seen
    width = SC.widest(vs)
    inc = [MapEdit(ADD, vs - width, width, 1)]
    # a key once, a key twice, a key 70 times across two waves, the absent ones in between
    batch = np.concatenate([pool[0:1], pool[1:2], absent[:2], np.repeat(pool[2:3], 35, axis=0), pool[1:2], absent[2:],
                            np.repeat(pool[2:3], 35, axis=0), pool[3:8]])
    check_modify_batch(lib, vm, twin, ref, m, dev, np.ascontiguousarray(batch), inc, host_form)
    check_modify_batch(lib, vm, twin, ref, m, dev, np.ascontiguousarray(batch), inc, host_form, want_vals=False, voff=1)  # the delete's FIND
    check_modify_batch(lib, vm, twin, ref, m, dev, np.ascontiguousarray(batch[::-1]), [MapEdit(SUB_SAT, 0, 1, 200), MapEdit(XOR, 0, 1, 1)], host_form,
                       want_found=False, koff=1, voff=4)
    # a following update and, on a HASH map, delete of the same keys behave as on a fresh table
    uk = np.unique(batch, axis=0)
    uk = np.ascontiguousarray(uk[MC.ref_lookup(ref, m, uk, vs)[1] != 0])
    nv = rng.integers(0, 256, size=(len(uk), vs), dtype=np.uint8)
    for v in (vm, twin):
        v.map_update_batch_device(m, dev(uk), dev(nv))
    MC.ref_update(ref, m, uk, nv)
    same_state(lib, vm, twin, m, dev, 100 if array else ref.map_count(m), "an update after the keyed modify")
    if not array:
        found = to_np(vm.map_delete_batch(m, dev(uk[:3].copy())))
        assert list(found) == [1, 1, 1] and list(to_np(twin.map_delete_batch(m, dev(uk[:3].copy())))) == [1, 1, 1]
        MC.ref_delete(ref, m, uk[:3])
        same_image_map(vm, ref, m, dev, "a delete after the keyed modify")
    same_map(vm, ref, m, "after the keyed modifies")
    close(vm, twin, ref)


def run_keyed_counts(lib, oracle_lib, dev, count: int, host_form: bool = False) -> None:
    """Batches of 1, 255, 256, 257 and 65,537 keys drawn from 40 present and 8 absent ones: at 65,537 every
    key is repeated more than a thousand times, in every workgroup of the launch."""
    rng = np.random.default_rng(9500 + count)
    ks, vs = 8, 24
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, _ = fill3(vm, twin, ref, m, dev, rng, ks, vs, 60)
    pool = np.concatenate([keys, MC.hash_pool(rng, ks, 8)])
    batch = np.ascontiguousarray(pool[rng.integers(0, len(pool), size=count)])
    check_modify_batch(lib, vm, twin, ref, m, dev, batch, [MapEdit(ADD, 16, 8, 1), MapEdit(ADD_SAT, 0, 2, 0x4000)], host_form)
    same_map(vm, ref, m, f"after a batch of {count}")
    close(vm, twin, ref)


# ---------------------------------------------------------------- 8. under traffic
def prog_gate() -> list[int]:
    """C3's lookup with a gate: a hit counts (hits += 1, atomic) and is dropped when the value's first field,
    its tokens, is 0, redirected otherwise; a miss passes."""
    a = Asm()
    W._parse_eth(a, "pass")
    a.jmp(JNE, 3, "pass", imm=0x0008)
    a.mov64(2, src=6).add64(2, src=4)
    a.mov64(5, src=2).add64(5, 24)
    a.jmp(JGT, 5, "pass", src=7)
    W._tuple_key(a)
    a.ld_map(1, 1)
    a.mov64(2, src=10).add64(2, -16)
    a.call(1)
    a.jmp(JEQ, 0, "pass", imm=0)
    a.mov64(1, 1)
    a.xadd(8, 0, 8, 1)                      # value.hits += 1
    a.ldx(8, 3, 0, 0)                       # tokens
    a.jmp(JEQ, 3, "drop", imm=0)
    a.mov64(0, XDP_REDIRECT)
    a.exit()
    a.label("drop")
    a.mov64(0, XDP_DROP)
    a.exit()
    a.label("pass")
    a.mov64(0, XDP_PASS)
    a.exit()
    return a.assemble()


def gate_vm(lib):
    vm = VM(Settings(engine=1), lib=lib)
    m = vm.add_map(MapDef(MAP_HASH, 16, 16, MC.FLOW_MAX))
    vm.set_entrypoint(vm.add_raw_program(prog_gate()))
    return vm, m


def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    """batch -> modify (the refill of the empty buckets) -> batch, with no xe_sync in between: the verdicts and
    the map are the oracle's given the same refill through its update, the state is the twin's, and the call
    neither downloads nor uploads the map."""
    (vm, m), (twin, _), (ref, rm) = gate_vm(lib), gate_vm(lib), gate_vm(oracle_lib)
    keys, vals = MC.flow_entries(list(range(24)) + [(1 << 41) + i for i in range(8)])
    vals[::2, 0:8] = 0  # every other bucket is empty: its packets are dropped
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    clone_state(vm, m, dev, twin)
    MC.ref_update(ref, rm, keys, vals)
    runs = [MC.Runner(vm, dev, use_async), MC.Runner(twin, dev, use_async)]

    def ref_run(start: int) -> np.ndarray:
        umem, descs = W.build_batch("c3learn", start, MC.FLOW_PACKETS)
        return ref.run_batch(umem, descs).verdicts

    v0 = [r.run(0) for r in runs]
    w0 = ref_run(0)
    assert (w0 == XDP_DROP).any() and (w0 == XDP_REDIRECT).any()
    traffic = vm.map_traffic(m)
    refill = [MapEdit(SET, 0, 8, 5)]
    empty = MapFilter(SC.EQ, 0, 8, 0)
    # no xe_sync in between: the call completes the pipeline itself
    k, v, matched, _ = modify_call(lib, vm, m, dev, empty, refill, MC.FLOW_MAX, 64)
    assert vm.map_traffic(m) == traffic, "the modify moved the whole map"
    assert np.array_equal(to_np(v0[0]), w0) and np.array_equal(to_np(v0[1]), w0)
    rk, rv = ref.map_dump(rm)
    sel = selects(rv, empty)
    assert matched == int(sel.sum()) == 16
    gk, gv = MC.by_key(k, v)
    wk, wv = MC.by_key(rk[sel], rv[sel])
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), "the refilled entries are not the oracle's empty buckets (hits included)"
    tk, tv, _ = twin.map_scan(m, empty)
    assert np.array_equal(tk, k) and np.array_equal(tv, v)
    new = edit_rows(v, refill)
    twin.map_update_batch_device(m, dev(np.ascontiguousarray(k)), dev(new))
    MC.ref_update(ref, rm, k, new)
    # the delta base follows the update's rule: the refilled entries' pending adds (the hits) are dropped, every other entry's stay
    _, _, _, delta = same_state(lib, vm, twin, m, dev, 32, "after the refill", with_delta=not use_async)
    if not use_async:
        snap = Snapshot(vm, ref, m, dev)
        dv = delta[:(int(snap.slots.max()) + 1) * 16].reshape(-1, 16)
        hit = np.array([bytes(x) in set(map(bytes, k)) for x in snap.keys])
        assert not dv[snap.slots[hit]].any(), "a refilled entry shows up in xe_map_delta"
        assert dv[snap.slots[~hit]].any(), "the batch's adds on the other entries are gone"
    v1 = [r.run(MC.FLOW_PACKETS) for r in runs]
    w1 = ref_run(MC.FLOW_PACKETS)
    assert not (w1 == XDP_DROP).any(), "the refill did not open the gate"
    same_image_map(vm, ref, m, dev, "after the second batch")  # (completes the pipeline)
    assert np.array_equal(to_np(v1[0]), w1) and np.array_equal(to_np(v1[1]), w1)
    assert vm.map_traffic(m) == traffic, "a batch after the device modify moved the map"
    # keyed, between batches: the first four buckets emptied again
    old, found = vm.map_modify_batch(m, dev(keys[:4].copy()), [MapEdit(SET, 0, 8, 0)])
    assert to_np(found).all()
    MC.ref_update(ref, rm, keys[:4], edit_rows(to_np(old), [MapEdit(SET, 0, 8, 0)]))
    v2 = runs[0].run(2 * MC.FLOW_PACKETS)
    w2 = ref_run(2 * MC.FLOW_PACKETS)
    same_map(vm, ref, m, "after three batches")
    assert np.array_equal(to_np(v2), w2) and (w2 == XDP_DROP).any()
    close(vm, twin, ref)


def modify_call(lib, vm, m, dev, flt, edits, cap: int, room: int):
    """A reporting walk call into plain buffers. Returns (keys[r], values[r], matched, None)."""
    d = vm.map_defs[m]
    ks, vs = (4 if d.type == MAP_ARRAY else d.key_size), d.value_size
    kbuf, vbuf = dev(np.full((room, ks), GUARD, np.uint8)), dev(np.full((room, vs), GUARD, np.uint8))
    settle(kbuf)
    rc, matched = raw_modify(lib, vm, m, flt, edits, addr(kbuf), addr(vbuf), cap, True)
    assert rc == 0, lib.last_error(vm.h)
    r = min(matched, cap)
    return to_np(kbuf)[:r].copy(), to_np(vbuf)[:r].copy(), matched, None


# ---------------------------------------------------------------- 9. epoch, limits, determinism
def run_epoch(lib, dev) -> None:
    vm, m = MC.flow_vm(lib)
    keys, vals = MC.flow_entries(range(8))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    before = state_image(vm, m, dev)
    edit = [MapEdit(ADD, 8, 8, 1)]
    d_k = dev(keys)
    settle(d_k)
    vm.epoch_begin()
    for device_form in (True, False):
        for cap in (0, 8):
            assert raw_modify(lib, vm, m, None, edit, 0, 0, cap, device_form)[0] == MC.ERR_INVAL
        kptr = addr(d_k) if device_form else keys.ctypes.data
        assert raw_modify_batch(lib, vm, m, kptr, 8, edit, 0, 0, device_form) == MC.ERR_INVAL
    assert b"epoch" in lib.last_error(vm.h)
    assert np.array_equal(before, state_image(vm, m, dev)), "a call refused in an epoch changed the map"
    vm.epoch_end()
    assert raw_modify(lib, vm, m, None, edit, 0, 0, 3, True) == (0, 8)
    got = to_np(vm.map_lookup_batch(m, dev(keys))[0])
    assert int((got[:, 8] == 1).sum()) == 3 and vm.map_count(m) == 8
    vm.close()


def run_limits(lib, oracle_lib, dev) -> None:
    ok = [MapEdit(ADD, 0, 1, 1)]
    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        m = vm.add_map(MapDef(t, 4, 8, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 8, 16))
        k, v = np.zeros((2, 4), np.uint8), np.zeros((2, 8), np.uint8)
        for device_form in (True, False):
            assert raw_modify(lib, vm, m, None, ok, k.ctypes.data, v.ctypes.data, 2, device_form)[0] == MC.ERR_UNSUPPORTED
            assert b"ARRAY and HASH" in lib.last_error(vm.h)
            assert raw_modify_batch(lib, vm, m, k.ctypes.data, 2, ok, v.ctypes.data, 0, device_form) == MC.ERR_UNSUPPORTED
        vm.close()

    vs = 13
    rng = np.random.default_rng(15)
    vm, ref, m, _ = MC.pair(lib, oracle_lib, MapDef(MAP_HASH, 8, vs, MC.HASH_MAX))
    keys, _ = fill_hash(vm, ref, m, dev, rng, 8, vs, 30)
    before = state_image(vm, m, dev)
    d_k = dev(keys)
    settle(d_k)
    E = N.MapEdit
    bad = [[E(11, 0, 1, 0, 0)], [E(0xffffffff, 0, 1, 0, 0)],                                    # an unknown op
           [E(ADD, 0, 1, 2, 0)], [E(ADD, 0, 1, 0x80000001, 0)],                                  # an unknown flag bit
           [E(ADD, 0, 0, 0, 0)], [E(ADD, 0, 3, 0, 0)], [E(ADD, 0, 16, 0, 0)],                    # width
           [E(ADD, vs, 1, 0, 0)], [E(ADD, vs - 7, 8, 0, 0)], [E(ADD, 0xffffffff, 8, 0, 0)], [E(ADD, 0xfffffffc, 4, 0, 0)],  # the field
           [E(ADD, 0, 1, 1, vs)], [E(ADD, 0, 8, 1, vs - 7)], [E(ADD, 0, 4, 1, M64)], [E(ADD, 0, 4, 1, M64 - 3)],          # the operand field
           [E(ADD, 0, 1, 1, 1 << 32)],
           [E(ADD, 0, 1, 0, 1), E(ADD, 0, 1, 0, 1), E(SHR, 0, 5, 0, 1)]]                         # a bad edit behind good ones
    calls = [([], dict()), (ok, dict(null_edits=True)), (ok, dict(n_edits=0)), (ok * (MAX_EDITS + 1), dict()), (ok, dict(n_edits=0xffffffff))]
    calls += [(b, dict()) for b in bad]
    for edits, kw in calls:
        for device_form in (True, False):
            kptr = addr(d_k) if device_form else keys.ctypes.data
            assert raw_modify(lib, vm, m, None, edits, 0, 0, 5, device_form, **kw)[0] == MC.ERR_INVAL, (len(edits), kw)
            assert raw_modify_batch(lib, vm, m, kptr, 5, edits, 0, 0, device_form, **kw) == MC.ERR_INVAL, (len(edits), kw)
            assert raw_modify_batch(lib, vm, m, 0, 0, edits, 0, 0, device_form, **kw) == MC.ERR_INVAL, (len(edits), kw)  # even for no keys
    for device_form in (True, False):
        kptr = addr(d_k) if device_form else keys.ctypes.data
        for f in (N.MapFilter(9, 0, 1, 0, 0), N.MapFilter(SC.EQ, 0, 1, 1, 0), N.MapFilter(SC.EQ, 0, 3, 0, 0), N.MapFilter(SC.EQ, vs, 1, 0, 0)):
            assert raw_modify(lib, vm, m, f, ok, 0, 0, 5, device_form)[0] == MC.ERR_INVAL  # the filter's errors
        assert raw_modify(lib, vm, m, None, ok, 0, 0, 5, device_form, matched=False)[0] == MC.ERR_INVAL  # a NULL matched
        assert raw_modify(lib, vm, 99, None, ok, 0, 0, 5, device_form)[0] == MC.ERR_INVAL  # a bad map index
        assert raw_modify_batch(lib, vm, m, 0, 5, ok, 0, 0, device_form) == MC.ERR_INVAL  # keys NULL with count > 0
        assert raw_modify_batch(lib, vm, m, kptr, (1 << 31) + 1, ok, 0, 0, device_form) == MC.ERR_INVAL
        assert raw_modify_batch(lib, vm, 99, kptr, 5, ok, 0, 0, device_form) == MC.ERR_INVAL
        assert raw_modify_batch(lib, vm, m, 0, 0, ok, 0, 0, device_form) == 0  # no keys: nothing to do
        assert raw_modify(lib, vm, m, None, ok, 0, 0, 0, device_form) == (0, 20)  # cap 0 only counts
    assert raw_modify(lib, vm, m, N.MapFilter(SC.ALL, 1000, 77, 0, 5), [E(ADD, 0, 1, 0, 0)], 0, 0, 0, True) == (0, 20)  # ALL ignores the field
    assert np.array_equal(before, state_image(vm, m, dev)), "a refused call changed the map"
    same_map(vm, ref, m, "after the refused calls")
    close(vm, ref)


def run_determinism(lib, dev) -> None:
    """Two identical VMs, the same calls: identical state bytes and identical reports."""
    rng = np.random.default_rng(16)
    ks, vs, n = 24, 65, 3000
    keys = MC.hash_pool(rng, ks, n)
    vals = rng.integers(0, 256, size=(n, vs), dtype=np.uint8)
    batch = np.ascontiguousarray(keys[rng.integers(0, n, size=5000)])
    out = []
    vms = [VM(Settings(engine=1), lib=lib) for _ in range(2)]
    m = [v.add_map(MapDef(MAP_HASH, ks, vs, 4096)) for v in vms][0]
    vms[0].map_update_batch_device(m, dev(keys), dev(vals))
    vms[0].map_delete_batch(m, dev(np.ascontiguousarray(keys[::3])))
    clone_state(vms[0], m, dev, vms[1])
    for vm in vms:
        edits = [MapEdit(ADD, 3, 8, 0x0102030405060708), MapEdit(SHR, 60, 4, 5), MapEdit(MAX, 1, 2, 61, True)]
        rep = modify_call(lib, vm, m, dev, MapFilter(SC.GT, 3, 4, 1 << 30), edits, 1500, 1500)
        assert raw_modify(lib, vm, m, MapFilter(SC.LE, 3, 4, 1 << 30), edits[:1], 0, 0, M64, True)[0] == 0
        old, found = vm.map_modify_batch(m, dev(batch), edits)
        out.append((rep[0], rep[1], rep[2], to_np(old).copy(), to_np(found).copy(), state_image(vm, m, dev)))
        vm.close()
    assert 500 < out[0][2] < 2000
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- the Python interface
def run_python_api(lib, oracle_lib, dev, on_device: bool) -> None:
    rng = np.random.default_rng(17)
    ks, vs = 8, 24
    vm, twin, ref, m = trio(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    keys, _ = fill3(vm, twin, ref, m, dev, rng, ks, vs, 40)
    snap = Snapshot(vm, ref, m, dev)
    flt = MapFilter(SC.ANYBITS, 2, 1, 1)
    ek, ev = snap.expect(flt)
    assert 5 <= len(ek) < len(snap.keys)
    edits = [MapEdit(ADD, 8, 8, 3), MapEdit(MIN, 8, 8, 16, operand_field=True)]

    def mirror(k, v):  # the twin and the oracle get the model's values
        new = edit_rows(v, edits)
        if len(k):
            twin.map_update_batch_device(m, dev(np.ascontiguousarray(k)), dev(new))
            MC.ref_update(ref, m, k, new)
        same_state(lib, vm, twin, m, dev, len(snap.keys), "the Python interface")
        same_image_map(vm, ref, m, dev, "the Python interface")

    k, v, matched = vm.map_modify(m, edits, flt, on_device=on_device)  # cap None: count first, then fetch all
    assert on_dev(k) == on_device and matched == len(ek) and np.array_equal(to_np(k), ek) and np.array_equal(to_np(v), ev)
    mirror(ek, ev)
    k, v, matched = vm.map_modify(m, edits, cap=3, on_device=on_device)
    assert matched == len(snap.keys) and np.array_equal(to_np(k), snap.keys[:3])
    mirror(to_np(k), to_np(v))
    tk, tv, _ = twin.map_scan(m, flt)  # (the edits leave byte 2 alone: the same entries match)
    assert vm.map_modify(m, edits, flt, on_device=on_device, report=False) == len(ek)
    mirror(tk, tv)
    batch = np.ascontiguousarray(np.concatenate([keys[:6], keys[1:2], keys[1:2]]))  # keys[0] and keys[3] were deleted
    old, found = vm.map_modify_batch(m, dev(batch) if on_device else batch, edits)
    assert on_dev(old) == on_device and list(to_np(found)) == [0, 1, 1, 0, 1, 1, 1, 1]
    wv, _ = MC.ref_lookup(ref, m, batch, vs)
    assert np.array_equal(to_np(old), wv)
    mirror(batch[[1, 2, 4, 5]], wv[[1, 2, 4, 5]])
    old, found = vm.map_modify_batch(m, batch[:2].copy(), edits, on_device=on_device)  # numpy keys, placed by on_device
    assert on_dev(old) == on_device and list(to_np(found)) == [0, 1]
    mirror(batch[1:2], to_np(old)[1:2])
    same_map(vm, ref, m, "the Python interface")
    # an ARRAY map: u32 indices
    am = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 10))
    vm.map_update(am, (7).to_bytes(4, "little"), b"\x05" * 8)
    k, v, matched = vm.map_modify(am, [MapEdit(SUB, 0, 1, 6)], MapFilter(SC.EQ, 0, 8, 0x0505050505050505), on_device=on_device)
    assert matched == 1 and to_np(k).view(np.uint32).tolist() == [[7]] and to_np(v).tolist() == [[5] * 8]
    assert vm.map_lookup(am, (7).to_bytes(4, "little")) == b"\xff" + b"\x05" * 7
    close(vm, twin, ref)
