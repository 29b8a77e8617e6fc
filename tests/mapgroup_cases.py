"""Shared cases of the device-side group-by (xe_map_group): tests/test_mapgroup.py runs them on the host
simulation, tests/test_mapgroup_gpu.py on the product library.

No expected value comes from the code under test:
  * the folded set is the source's mapscan_cases.Snapshot (the oracle's entries, checked against the exported
    image) filtered by mapscan_cases.selects;
  * the groups are a Python dict over the key and value bytes of that set (expect_groups), pinned by the
    hand-worked GROUP_TABLE;
  * for each group the oracle VM gets one map_update whose value is what its map_lookup returned (zeros if
    absent) with the two accumulators raised modulo 2^64; the destination must then equal the oracle through
    the exported image (same_image_map: no host visit) and through the dump (same_map);
  * created is the growth of the oracle's map_count; the source's image must not change at all.

Sizes (xe_mapops.h / xe_mapops.hip): a tile is 256 slots in 4 rounds of 64 lanes; the tile launcher gives
every tile a wave of its own up to 256 workgroups of 4 waves, then a quarter of that, so the 2,048 tiles of a
2^19-slot source are strided over by 1,024 waves; GROUP_ADD combines the lanes of a round for kMgLeaders = 4
distinct destination slots and lets the rest add singly, so 2, 3 and 9 groups a round sit on both sides of it;
destination records have 2, 4, 8 or 16 words (key sizes 3 / 4, 13 / 24, 64) and values of up to 16 bytes are
zeroed by one lane, larger ones by a wave."""
from __future__ import annotations

import ctypes as C

import numpy as np

import mapops_cases as MC
import mapscan_cases as SC
from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, MG_KEY, MG_NONE,
                                  MG_VALUE, VM, MapDef, MapFilter, MapGroup, MapOrder, Settings)
from mapops_cases import (GUARD, addr, flow_vm, hash_pool, home_slot, image_records, keys_with_home, pair, same_image_map, same_map,
                          settle, state_image, to_np, Runner)
from mapscan_cases import ALL, ANYBITS, EQ, GT, M64, NE, OPS, Snapshot, fields, selects

EDGE_COUNTS = (1, 63, 64, 65, 255, 256, 257)
FEW_GROUPS = (2, 3, 9)
KEY_SHAPES = ((MG_KEY, 0, 4), (MG_KEY, 1, 3), (MG_KEY, 3, 13), (MG_KEY, 0, 64),
              (MG_VALUE, 1, 3), (MG_VALUE, 5, 4), (MG_VALUE, 3, 13), (MG_VALUE, 7, 24), (MG_VALUE, 1, 64))
DST_VALUE_SIZES = (8, 16, 32, 4096)
ACCUMULATORS = ((0, 8), (8, 0), (16, MG_NONE), (MG_NONE, 24))  # (count_off, sum_off)
SHAPE_SRC_VS = 72  # the source value of the key-shape cases: room for 64 group bytes at +1 and a measure at vs - 8


# ---------------------------------------------------------------- the groups, restated
def expect_groups(keys: np.ndarray, vals: np.ndarray, g: MapGroup) -> dict:
    """{group bytes: (entries, sum of measures mod 2^64)} over the folded entries' key and value rows."""
    src = keys if g.from_ == MG_KEY else vals
    out: dict[bytes, tuple[int, int]] = {}
    for i in range(len(src)):
        gk = src[i, g.offset:g.offset + g.len].tobytes()
        meas = int.from_bytes(vals[i, g.measure_off:g.measure_off + g.measure_width].tobytes(), "little") if g.measure_width else 0
        c, s = out.get(gk, (0, 0))
        out[gk] = (c + 1, (s + meas) & M64)
    return out


def _rows(*rows):
    return np.array(rows, dtype=np.uint8)


# (keys, values, spec, groups), worked out by hand
GROUP_TABLE = (
    # by key bytes 1..2; the measure is value byte 0
    (_rows((9, 1, 2, 7), (8, 1, 2, 6), (9, 3, 2, 7)), _rows((5, 0), (250, 0), (1, 9)), MapGroup(MG_KEY, 1, 2, 0, 8, 0, 1),
     {b"\x01\x02": (2, 255), b"\x03\x02": (1, 1)}),
    # by value byte 1, no measure
    (_rows((9, 1, 2, 7), (8, 1, 2, 6), (9, 3, 2, 7)), _rows((5, 0), (250, 0), (1, 9)), MapGroup(MG_VALUE, 1, 1, 0, MG_NONE, 0, 0),
     {b"\x00": (2, 0), b"\x09": (1, 0)}),
    # a 2-byte little-endian measure at +1; the sum of two all-ones 8-byte measures wraps
    (_rows((1,), (1,)), _rows((0, 0x34, 0x12), (0, 0xff, 0xff)), MapGroup(MG_KEY, 0, 1, 0, 8, 1, 2), {b"\x01": (2, 0x1234 + 0xffff)}),
    (_rows((1,), (1,), (2,)), _rows((255,) * 8, (255,) * 8, (3,) + (0,) * 7), MapGroup(MG_KEY, 0, 1, 0, 8, 0, 8),
     {b"\x01": (2, M64 - 1), b"\x02": (1, 3)}),
    (np.zeros((0, 4), np.uint8), np.zeros((0, 8), np.uint8), MapGroup(MG_KEY, 0, 4, 0, 8, 0, 8), {}),
)


def check_group_table() -> None:
    for keys, vals, g, want in GROUP_TABLE:
        assert expect_groups(keys, vals, g) == want, (g, expect_groups(keys, vals, g))


# ---------------------------------------------------------------- the call and its check
def c_filter(flt):
    return None if flt is None else (flt if isinstance(flt, N.MapFilter) else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand))


def c_group(g):
    if g is None or isinstance(g, N.MapGroup):
        return g
    return N.MapGroup(g.from_, g.offset, g.len, g.measure_off, g.measure_width, g.count_off, g.sum_off, 0)


def raw_group(lib, vm: VM, src: int, flt, g, dst: int, matched=True, created=True):
    """One call. Returns (rc, matched, created)."""
    cf, cg = c_filter(flt), c_group(g)
    n, new = C.c_uint64(0xDEADBEEF), C.c_uint64(0xDEADBEEF)
    rc = lib.map_group(vm.h, src, None if cf is None else C.byref(cf), None if cg is None else C.byref(cg), dst,
                       C.byref(n) if matched else None, C.byref(new) if created else None, None)
    return rc, n.value, new.value


def dst_key(vm: VM, dst: int, gk: bytes) -> bytes:
    return gk if vm.map_defs[dst].type == MAP_HASH else int.from_bytes(gk, "little").to_bytes(4, "little")


def oracle_fold(ref: VM, dst: int, groups: dict, g: MapGroup) -> None:
    """One map_update per group: the oracle's own value (zeros if absent) with the accumulators raised."""
    vs = ref.map_defs[dst].value_size
    for gk, (c, s) in groups.items():
        key = dst_key(ref, dst, gk)
        v = bytearray(ref.map_lookup(dst, key) or bytes(vs))
        for off, add in ((g.count_off, c), (g.sum_off, s)):
            if off != MG_NONE:
                v[off:off + 8] = ((int.from_bytes(v[off:off + 8], "little") + add) & M64).to_bytes(8, "little")
        ref.map_update(dst, key, bytes(v))


def same_dst(vm: VM, ref: VM, dst: int, dev, what: str, host_visit: bool = True):
    """The destination against the oracle without a host visit (the image), then with one (the dump)."""
    if vm.map_defs[dst].type == MAP_HASH:
        img = same_image_map(vm, ref, dst, dev, what)
    else:
        img = state_image(vm, dst, dev)
        want = np.frombuffer(ref.map_dump(dst), dtype=np.uint8)
        assert np.array_equal(img[:len(want)], want), f"{what}: ARRAY values differ"
    if host_visit:
        same_map(vm, ref, dst, what)
    return img


def check_group(lib, vm: VM, ref: VM, src: int, dst: int, dev, g: MapGroup, flt=None, snap: Snapshot | None = None,
                host_visit: bool = True, what: str = ""):
    """A group call against the source's snapshot and the oracle's fold. Returns (matched, created, groups)."""
    snap = snap or Snapshot(vm, ref, src, dev)
    snap.expect(flt)  # the folded set is the oracle's
    sel = selects(snap.vals, flt)
    groups = expect_groups(snap.keys[sel], snap.vals[sel], g)
    hash_dst = vm.map_defs[dst].type == MAP_HASH
    had = ref.map_count(dst) if hash_dst else 0
    src_img = state_image(vm, src, dev)
    rc, matched, created = raw_group(lib, vm, src, flt, g, dst)
    what = what or f"group {g} filter {flt}"
    assert rc == 0, f"{what}: {lib.last_error(vm.h)}"
    assert matched == int(sel.sum()) == sum(c for c, _ in groups.values()), f"{what}: matched {matched}, expected {int(sel.sum())}"
    oracle_fold(ref, dst, groups, g)
    want_new = ref.map_count(dst) - had if hash_dst else 0
    assert created == want_new, f"{what}: created {created}, expected {want_new}"
    assert np.array_equal(src_img, state_image(vm, src, dev)), f"{what}: the source changed"
    same_dst(vm, ref, dst, dev, what, host_visit)
    return matched, created, groups


def two_maps(lib, oracle_lib, sdef: MapDef, ddef: MapDef):
    vm, ref, src, _ = pair(lib, oracle_lib, sdef)
    return vm, ref, src, (vm.add_map(ddef), ref.add_map(ddef))[0]


def install(vm: VM, ref: VM, m: int, dev, keys: np.ndarray, vals: np.ndarray) -> None:
    vm.map_update_batch_device(m, dev(np.ascontiguousarray(keys)), dev(np.ascontiguousarray(vals)))
    MC.ref_update(ref, m, keys, vals)


def remove(vm: VM, ref: VM, m: int, dev, keys: np.ndarray) -> None:
    assert to_np(vm.map_delete_batch(m, dev(np.ascontiguousarray(keys)))).all()
    MC.ref_delete(ref, m, keys)


def array_rows(n: int) -> np.ndarray:
    return np.arange(n, dtype=np.uint32).view(np.uint8).reshape(-1, 4).copy()


def u64_rows(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64)).view(np.uint8).reshape(-1, 8)


# ---------------------------------------------------------------- 1. tile and round edges
def run_edges(lib, oracle_lib, dev, live: int) -> None:
    """`live` entries among the tombstones of half as many deleted ones: each its own group (by the whole key),
    then all in one group (by a value byte they share)."""
    rng = np.random.default_rng(1000 + live)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, 512), MapDef(MAP_HASH, 8, 16, 512))
    one = vm.add_map(MapDef(MAP_HASH, 1, 16, 4))
    ref.add_map(MapDef(MAP_HASH, 1, 16, 4))
    extra = (live + 1) // 2
    keys = hash_pool(rng, 8, live + extra)
    vals = rng.integers(0, 256, size=(len(keys), 16), dtype=np.uint8)
    vals[:, 15] = 0x5c
    install(vm, ref, src, dev, keys, vals)
    remove(vm, ref, src, dev, keys[live:])
    snap = Snapshot(vm, ref, src, dev)
    assert len(snap.keys) == live and snap.tombs == extra
    matched, created, groups = check_group(lib, vm, ref, src, dst, dev, MapGroup(MG_KEY, 0, 8, 0, 8, 0, 8), snap=snap)
    assert (matched, created, len(groups)) == (live, live, live)
    matched, created, groups = check_group(lib, vm, ref, src, one, dev, MapGroup(MG_VALUE, 15, 1, 8, 0, 4, 4), snap=snap)
    assert (matched, created) == (live, 1) and groups[b"\x5c"][0] == live
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. striding waves
def run_striding(lib, oracle_lib, dev) -> None:
    """A source of 2^19 slots, about half full, by a 2-byte field of 1,500 distinct values: 2,048 tiles for
    1,024 waves, and rounds that mix many groups."""
    slots, n = 1 << 19, 250_000
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 8, slots // 2), MapDef(MAP_HASH, 2, 16, 2048))
    assert MC.hash_geometry(vm, src)[0] == slots
    c = np.arange(1, n + 1, dtype=np.uint64)
    keys = u64_rows(c)
    vals = u64_rows(((c * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(1500) + (c << np.uint64(16)))
    vm.map_update_batch_device(src, dev(keys), dev(vals))
    # (the oracle is not given 250,000 entries one by one: the folded set is the installed arrays, which the
    # device lookups below tie to the map)
    got, found = vm.map_lookup_batch(src, dev(keys[::997].copy()))
    assert to_np(found).all() and np.array_equal(to_np(got), vals[::997])
    g = MapGroup(MG_VALUE, 0, 2, 0, 8, 2, 4)
    groups = expect_groups(keys, vals, g)
    assert len(groups) == 1500
    src_img = state_image(vm, src, dev)
    rc, matched, created = raw_group(lib, vm, src, None, g, dst)
    assert (rc, matched, created) == (0, n, 1500), lib.last_error(vm.h)
    oracle_fold(ref, dst, groups, g)
    assert np.array_equal(src_img, state_image(vm, src, dev)), "the source changed"
    same_dst(vm, ref, dst, dev, "2^19 slots by a 2-byte field")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. one hot group
def run_hot(lib, oracle_lib, dev) -> None:
    """4,099 ARRAY entries and two whose 8-byte measure is all ones into one destination entry: the sum wraps."""
    n = 4101
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 16, n), MapDef(MAP_HASH, 1, 16, 4))
    vals = np.zeros((n, 16), np.uint8)
    meas = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(3)
    meas[[77, 4000]] = np.uint64(M64)
    vals[:, 8:16] = u64_rows(meas)
    vals[:, 3] = 0xa7
    install(vm, ref, src, dev, array_rows(n), vals)
    matched, created, groups = check_group(lib, vm, ref, src, dst, dev, MapGroup(MG_VALUE, 3, 1, 0, 8, 8, 8))
    total = sum(int(x) for x in meas) & M64
    assert (matched, created) == (n, 1) and groups == {b"\xa7": (n, total)}
    got = vm.map_lookup(dst, b"\xa7")
    assert int.from_bytes(got[:8], "little") == n and int.from_bytes(got[8:], "little") == total
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 4. few groups
def run_few(lib, oracle_lib, dev, ngroups: int) -> None:
    """ngroups groups interleaved slot by slot (an ARRAY source: the slot is the index). ngroups 0: lanes 0 .. 62
    of every round share a group and lane 63 has another."""
    n = 700
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 12, n), MapDef(MAP_ARRAY, 4, 16, 16))
    i = np.arange(n)
    vals = np.zeros((n, 12), np.uint8)
    vals[:, 5] = i % ngroups if ngroups else (i % 64 == 63) * 11
    vals[:, 1:5] = ((i * 2654435761) & 0xffffffff).astype(np.uint32).view(np.uint8).reshape(-1, 4)
    install(vm, ref, src, dev, array_rows(n), vals)
    matched, created, groups = check_group(lib, vm, ref, src, dst, dev, MapGroup(MG_VALUE, 5, 1, 8, 0, 1, 4))
    assert (matched, created, len(groups)) == (n, 0, ngroups or 2)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 5. claim races
def run_chain(lib, oracle_lib, dev) -> None:
    """A destination table of 16 slots; eight group keys that all have their home in slot 14, so their chain
    wraps the end of the table; 600 source entries race for the eight records."""
    ks = 8
    want = {s for s in range(MC.HASH_CAP) if s & 15 == 14}
    gkeys = keys_with_home(ks, want, 8)
    assert all(home_slot(k, 16) == 14 for k in gkeys)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 24, 1024), MapDef(MAP_HASH, ks, 16, 8))
    assert MC.hash_geometry(vm, dst)[0] == 16
    rng = np.random.default_rng(55)
    n = 600
    keys = hash_pool(rng, 8, n)
    vals = rng.integers(0, 256, size=(n, 24), dtype=np.uint8)
    which = rng.integers(0, 8, size=n)
    vals[:, 9:17] = np.array([np.frombuffer(gkeys[w], np.uint8) for w in which])
    install(vm, ref, src, dev, keys, vals)
    matched, created, groups = check_group(lib, vm, ref, src, dst, dev, MapGroup(MG_VALUE, 9, 8, 8, 0, 17, 4), host_visit=False)
    assert (matched, created, len(groups)) == (n, 8, 8)
    w0 = image_records(vm, dst, state_image(vm, dst, dev))[0]
    full = set(np.nonzero(w0[:16] & np.uint64(MC.SLOT_FULL))[0].tolist())
    assert full == {14, 15, 0, 1, 2, 3, 4, 5}, f"the chain from slot 14 did not wrap: {sorted(full)}"
    same_map(vm, ref, dst, "after the wrapping chain")
    vm.close()
    ref.close()


FIT_GROUPS, FIT_OLD = 3000, 40


def run_fit(lib, oracle_lib, dev, room: int) -> None:
    """3,000 distinct new groups and hits on 40 pre-existing entries into a destination with `room` free
    entries: exactly 3,000 fit; with 2,999 the call fails and both maps are bit for bit what they were."""
    rng = np.random.default_rng(66)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 8, 4096), MapDef(MAP_HASH, 4, 24, FIT_OLD + room))
    gk = hash_pool(rng, 4, FIT_GROUPS + FIT_OLD)
    old = gk[FIT_GROUPS:]
    old_vals = rng.integers(0, 256, size=(FIT_OLD, 24), dtype=np.uint8)
    install(vm, ref, dst, dev, old, old_vals)
    n = FIT_GROUPS + 2 * FIT_OLD + 500
    keys = hash_pool(rng, 8, n)
    vals = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    vals[:FIT_GROUPS + FIT_OLD, 0:4] = gk
    vals[FIT_GROUPS + FIT_OLD:, 0:4] = gk[rng.integers(0, len(gk), size=n - len(gk))]
    install(vm, ref, src, dev, keys, vals)
    g = MapGroup(MG_VALUE, 0, 4, 8, 16, 4, 4)
    if room >= FIT_GROUPS:
        matched, created, _ = check_group(lib, vm, ref, src, dst, dev, g)
        assert (matched, created) == (n, FIT_GROUPS)
        for k, v in zip(old, old_vals):  # a pre-existing entry's other bytes are untouched
            assert vm.map_lookup(dst, k.tobytes())[:8] == v[:8].tobytes()
    else:
        before = state_image(vm, src, dev), state_image(vm, dst, dev)
        assert raw_group(lib, vm, src, None, g, dst)[0] == MC.ERR_NOMEM
        assert np.array_equal(before[0], state_image(vm, src, dev)), "a refused call changed the source"
        assert np.array_equal(before[1], state_image(vm, dst, dev)), "a refused call changed the destination"
        same_map(vm, ref, src, "source after XE_ERR_NOMEM")
        same_dst(vm, ref, dst, dev, "destination after XE_ERR_NOMEM")
    vm.close()
    ref.close()


def run_array_range(lib, oracle_lib, dev) -> None:
    """An ARRAY destination of 200 entries and a 1-byte group that reaches 255."""
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 8, 300), MapDef(MAP_ARRAY, 4, 8, 200))
    vals = np.zeros((300, 8), np.uint8)
    vals[:, 0] = np.arange(300) % 256
    install(vm, ref, src, dev, array_rows(300), vals)
    some = np.full((3, 8), 7, np.uint8)
    install(vm, ref, dst, dev, array_rows(3), some)
    before = state_image(vm, src, dev), state_image(vm, dst, dev)
    g = MapGroup(MG_VALUE, 0, 1, 0, MG_NONE, 0, 0)
    assert raw_group(lib, vm, src, None, g, dst)[0] == MC.ERR_INVAL
    assert np.array_equal(before[0], state_image(vm, src, dev)) and np.array_equal(before[1], state_image(vm, dst, dev))
    same_map(vm, ref, src, "source after an index out of range")
    same_dst(vm, ref, dst, dev, "destination after an index out of range")
    # the entries below 200 alone fold
    matched, created, _ = check_group(lib, vm, ref, src, dst, dev, g, MapFilter(SC.LT, 0, 1, 200))
    assert (matched, created) == (200 + 44, 0)  # indices 0 .. 199 and 256 .. 299
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 6. tombstone reuse
def run_tombstone_reuse(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(77)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 13, 16, 256), MapDef(MAP_HASH, 5, 16, 128))
    keys = hash_pool(rng, 13, 200)
    keys[:, 2:7] = keys[rng.integers(0, 90, size=200), 2:7]  # at most 90 groups
    keys = np.unique(keys, axis=0)
    vals = rng.integers(0, 256, size=(len(keys), 16), dtype=np.uint8)
    install(vm, ref, src, dev, keys, vals)
    g = MapGroup(MG_KEY, 2, 5, 0, 8, 3, 2)
    _, created, groups = check_group(lib, vm, ref, src, dst, dev, g, host_visit=False)
    first = Snapshot(vm, ref, dst, dev)
    assert created == len(groups) == len(first.keys) and first.tombs == 0
    gone = vm.map_expire(dst, None)[0]
    MC.ref_delete(ref, dst, to_np(gone))
    assert Snapshot(vm, ref, dst, dev).tombs == created
    up_down = vm.map_traffic(dst)
    _, again, _ = check_group(lib, vm, ref, src, dst, dev, g, host_visit=False)
    second = Snapshot(vm, ref, dst, dev)
    assert again == created and second.tombs == 0
    assert np.array_equal(second.slots, first.slots) and np.array_equal(second.keys, first.keys), "a group did not take its old record"
    assert np.array_equal(second.vals, first.vals)
    assert vm.map_traffic(dst) == up_down, "the destination was compacted through the host"
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 7. key shapes
def run_key_shape(lib, oracle_lib, dev, shape) -> None:
    """One group shape (from, offset, len) against every measure (width 1, 2, 4, 8 at 0, 1, 3, vs - width) and
    every accumulator layout that fits each destination value size; the calls accumulate into four
    destinations, one per value size, and each is compared after every call."""
    frm, off, ln = shape
    rng = np.random.default_rng(7000 + 100 * off + ln + frm)
    svs, n = SHAPE_SRC_VS, 40
    vm, ref, src, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 64, svs, 64))
    dsts = []
    for dvs in DST_VALUE_SIZES:
        dsts.append(vm.add_map(MapDef(MAP_HASH, ln, dvs, 64)))
        ref.add_map(MapDef(MAP_HASH, ln, dvs, 64))
    keys = hash_pool(rng, 64, n)
    vals = rng.integers(0, 256, size=(n, svs), dtype=np.uint8)
    rep = rng.integers(0, 12, size=n)  # about a dozen groups
    if frm == MG_KEY:
        keys[:, off:off + ln] = keys[rep, off:off + ln]
        keys = np.unique(keys, axis=0)
        vals = vals[:len(keys)]
    else:
        vals[:, off:off + ln] = vals[rep, off:off + ln]
    install(vm, ref, src, dev, keys, vals)
    snap = Snapshot(vm, ref, src, dev)
    calls = 0
    for width in (1, 2, 4, 8):
        for moff in (0, 1, 3, svs - width):
            for d, dvs in zip(dsts, DST_VALUE_SIZES):
                # (none of the four layouts fits an 8-byte value: it gets the one that does)
                for count_off, sum_off in (ACCUMULATORS if dvs > 8 else ((0, MG_NONE),)):
                    if any(o != MG_NONE and o + 8 > dvs for o in (count_off, sum_off)):
                        continue
                    g = MapGroup(frm, off, ln, count_off, sum_off, moff, width)
                    matched, _, groups = check_group(lib, vm, ref, src, d, dev, g, snap=snap, host_visit=False)
                    assert matched == len(snap.keys) and 2 <= len(groups) <= 12, (matched, len(snap.keys), len(groups))
                    calls += 1
    assert calls == 16 * (1 + 2 + 4 + 4)
    for d in dsts:
        same_map(vm, ref, d, f"shape {shape}")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 8. ARRAY sides
def run_array_sides(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(88)
    # ARRAY source -> HASH destination, by a value field
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_ARRAY, 4, 12, 777), MapDef(MAP_HASH, 3, 16, 64))
    vals = rng.integers(0, 256, size=(777, 12), dtype=np.uint8)
    vals[:, 1:4] = vals[rng.integers(0, 30, size=777), 1:4]
    install(vm, ref, src, dev, array_rows(777), vals)
    matched, created, groups = check_group(lib, vm, ref, src, dst, dev, MapGroup(MG_VALUE, 1, 3, 8, 0, 4, 8))
    assert matched == 777 and created == len(groups) <= 30
    # ... and by its own index bytes, at every offset
    for off, ln, entries in ((0, 1, 256), (1, 1, 4), (2, 2, 1), (3, 1, 1), (0, 2, 777), (0, 4, 777)):
        d = vm.add_map(MapDef(MAP_ARRAY, 4, 8, entries))
        ref.add_map(MapDef(MAP_ARRAY, 4, 8, entries))
        matched, created, groups = check_group(lib, vm, ref, src, d, dev, MapGroup(MG_KEY, off, ln, 0, MG_NONE, 0, 0))
        assert (matched, created) == (777, 0) and len(groups) == (777 if ln > 1 and off == 0 else min(256, entries))
    vm.close()
    ref.close()
    # HASH source -> ARRAY(256) by one byte, -> ARRAY(65,536) by two
    vm, ref, src, hist = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 16, 16, 1024), MapDef(MAP_ARRAY, 4, 16, 256))
    wide = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 65536))
    ref.add_map(MapDef(MAP_ARRAY, 4, 8, 65536))
    keys, vals = SC.fill_hash(vm, ref, src, dev, rng, 16, 16, 900)
    matched, created, groups = check_group(lib, vm, ref, src, hist, dev, MapGroup(MG_KEY, 9, 1, 0, 8, 7, 8))
    assert (matched, created) == (600, 0) and len(groups) > 200
    matched, created, groups = check_group(lib, vm, ref, src, wide, dev, MapGroup(MG_VALUE, 13, 2, 0, MG_NONE, 0, 0))
    assert (matched, created) == (600, 0) and max(int.from_bytes(k, "little") for k in groups) > 60000
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 9. nil-backed values
def run_vlen0(lib, oracle_lib, dev) -> None:
    """mapscan_cases.run_vlen0's setup: three of the four entries (keys 0 .. 3) of a HASH map are nil-backed.
    As a source they fold as zeros; as a destination a nil-backed entry ends as zeros + the group."""
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
    live = snap.vals[snap.vals.any(axis=1)]
    assert len(live) == 1
    # a source: the three nil-backed entries are one group (value bytes 0 0) with measure 0
    matched, created, groups = check_group(lib, vm, ref, m, by_val, dev, MapGroup(MG_VALUE, 0, 2, 0, 8, 0, 8), snap=snap)
    assert matched == 4 and groups[b"\0\0"] == (3, 0) and created == len(groups) == 2
    # a destination: indices 0 .. 5 of an ARRAY fold into keys 0 .. 3 (nil-backed or not) and two new ones
    install(vm, ref, feed, dev, array_rows(6), np.full((6, 8), 3, np.uint8))
    matched, created, _ = check_group(lib, vm, ref, feed, m, dev, MapGroup(MG_KEY, 0, 4, 0, MG_NONE, 0, 0), host_visit=False)
    assert (matched, created) == (6, 2)
    w0, keys, vals, _ = image_records(vm, m, state_image(vm, m, dev))
    assert not (w0 & np.uint64(MC.SLOT_VLEN0)).any(), "a folded record is still marked nil-backed"
    counts = sorted(int.from_bytes(v.tobytes(), "little") for v in vals[(w0 & np.uint64(MC.SLOT_FULL)) != 0])
    assert counts == [1, 1, 1, 1, 1, int.from_bytes(live[0].tobytes(), "little") + 1]
    same_map(vm, ref, m, "after folding into nil-backed entries")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 10. filters, accumulation
def run_filters(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(1010)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 13, 24, MC.HASH_MAX), MapDef(MAP_HASH, 1, 16, 256))
    SC.fill_hash(vm, ref, src, dev, rng, 13, 24, 60)
    snap = Snapshot(vm, ref, src, dev)
    live = len(snap.keys)
    operand = int(fields(snap.vals, 16, 8)[live // 2])
    g = MapGroup(MG_KEY, 4, 1, 0, 8, 9, 4)
    count = {}
    for op in OPS:
        count[op] = check_group(lib, vm, ref, src, dst, dev, g, MapFilter(op, 16, 8, operand), snap=snap)[0]
    assert count[ALL] == live and count[EQ] == 1 and count[NE] == live - 1 and count[SC.GE] + count[SC.LT] == live
    before = state_image(vm, dst, dev)
    assert raw_group(lib, vm, src, MapFilter(GT, 0, 1, 0xfff), g, dst) == (0, 0, 0)
    assert np.array_equal(before, state_image(vm, dst, dev)), "a group of nothing changed the destination"
    same_dst(vm, ref, dst, dev, "after a group of nothing")
    vm.close()
    ref.close()


def run_accumulation(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(1111)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, 512), MapDef(MAP_HASH, 1, 16, 256))
    keys, vals = SC.fill_hash(vm, ref, src, dev, rng, 8, 16, 300, delete_third=False)
    g = MapGroup(MG_KEY, 0, 1, 0, 8, 8, 8)
    _, created, groups = check_group(lib, vm, ref, src, dst, dev, g)
    once = {k: vm.map_lookup(dst, k) for k in groups}
    assert check_group(lib, vm, ref, src, dst, dev, g)[1] == 0
    for k, (c, s) in groups.items():  # two identical calls double the accumulators
        v = vm.map_lookup(dst, k)
        assert int.from_bytes(v[:8], "little") == 2 * c and int.from_bytes(v[8:], "little") == (2 * s) & M64
        assert int.from_bytes(once[k][:8], "little") == c
    # the source's values change on the device: the next call folds the new ones
    vals[:100, 8:16] = rng.integers(0, 256, size=(100, 8), dtype=np.uint8)
    install(vm, ref, src, dev, keys[:100], vals[:100])
    other = vm.add_map(MapDef(MAP_HASH, 1, 16, 256))
    ref.add_map(MapDef(MAP_HASH, 1, 16, 256))
    _, _, fresh = check_group(lib, vm, ref, src, other, dev, g)
    assert fresh != groups and {k: c for k, (c, _) in fresh.items()} == {k: c for k, (c, _) in groups.items()}
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 11. beside traffic
def ranked(keys: np.ndarray, vals: np.ndarray, off: int):
    f = fields(vals, off, 8)
    order = np.lexsort((np.arange(len(f)), ~f))
    return keys[order], vals[order]


def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    """Top talkers by source, end to end: a pipelined batch, map_group by the first four key bytes with no
    xe_sync in between, map_top over the result."""
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    ddef = MapDef(MAP_HASH, 4, 16, MC.FLOW_MAX)
    dst = vm.add_map(ddef)
    assert ref.add_map(ddef) == dst and rm == m
    r = Runner(vm, dev, use_async)
    keys, vals = MC.flow_entries(list(range(48)))
    install(vm, ref, m, dev, keys, vals)
    v0 = r.run(0)
    umem, descs = MC.W.build_batch("c3learn", 0, MC.FLOW_PACKETS)
    w0 = ref.run_batch(umem, descs).verdicts
    traffic = vm.map_traffic(m), vm.map_traffic(dst)
    g = MapGroup(MG_KEY, 0, 4, 0, 8, 8, 8)  # flows and packets (the hit counter) per source address
    rc, matched, created = raw_group(lib, vm, m, None, g, dst)  # completes the pipeline itself
    assert rc == 0, lib.last_error(vm.h)
    assert np.array_equal(to_np(v0), w0)
    rk, rv = ref.map_dump(rm)
    groups = expect_groups(rk, rv, g)
    assert matched == len(rk) and created == len(groups) and created > 1
    oracle_fold(ref, dst, groups, g)
    k, v, n, cut = vm.map_top(dst, MapOrder(8, 8, True), 5, ranked=False)
    assert (vm.map_traffic(m), vm.map_traffic(dst)) == traffic, "a group or a top moved a whole map"
    # nothing of the fold shows as packet adds
    out = dev(np.full(vm.map_values_bytes(dst), GUARD, np.uint8))
    settle(out)
    vm.map_delta(dst, addr(out), lane=8)
    assert not to_np(out)[:(MC.hash_geometry(vm, dst)[0] + 1) * 16].any(), "the fold shows up in xe_map_delta"
    snap = Snapshot(vm, ref, dst, dev)
    wk, wv = ranked(snap.keys, snap.vals, 8)
    want_cut = int(fields(wv[:5], 8, 8)[-1])
    gk, gv = ranked(to_np(k), to_np(v), 8)
    assert n == len(groups) and cut == want_cut
    assert np.array_equal(fields(gv, 8, 8), fields(wv[:5], 8, 8)), "the top talkers' packet counts differ"
    assert {bytes(x) for x in gk[fields(gv, 8, 8) > np.uint64(want_cut)]} == {bytes(x) for x in wk[:5][fields(wv[:5], 8, 8) > np.uint64(want_cut)]}
    same_map(vm, ref, dst, "the per-source table")
    # a host write to the source, then a group: exactly one upload
    nk, _ = MC.flow_entries([1 << 40])
    vm.map_update(m, nk[0].tobytes(), b"\x01" * 16)
    ref.map_update(rm, nk[0].tobytes(), b"\x01" * 16)
    up = vm.map_traffic(m)[0]
    matched2, _, _ = check_group(lib, vm, ref, m, dst, dev, g)
    assert matched2 == matched + 1 and vm.map_traffic(m)[0] == up + 1
    assert raw_group(lib, vm, m, None, g, dst)[0] == 0 and vm.map_traffic(m)[0] == up + 1
    vm.close()
    ref.close()


def run_epoch(lib, dev) -> None:
    vm, m = flow_vm(lib)
    dst = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 256))
    keys, vals = MC.flow_entries(range(8))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    g = MapGroup(MG_VALUE, 0, 1, 0, MG_NONE, 0, 0)
    vm.epoch_begin()
    assert raw_group(lib, vm, m, None, g, dst)[0] == MC.ERR_INVAL
    vm.epoch_end()
    assert raw_group(lib, vm, m, None, g, dst) == (0, 8, 0)
    hist = np.frombuffer(vm.map_dump(dst), dtype=np.uint64)
    assert hist[1:9].tolist() == [1] * 8 and int(hist.sum()) == 8
    vm.close()


# ---------------------------------------------------------------- 12. limits
def run_limits(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(1212)
    good = N.MapGroup(MG_VALUE, 0, 4, 0, 4, 0, 8, 0)
    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        bad = vm.add_map(MapDef(t, 4, 16, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 16, 16))
        ok = vm.add_map(MapDef(MAP_HASH, 4, 16, 16))
        for s, d in ((bad, ok), (ok, bad)):
            assert raw_group(lib, vm, s, None, good, d)[0] == MC.ERR_UNSUPPORTED, (t, s, d)
            assert b"ARRAY and HASH" in lib.last_error(vm.h)
        vm.close()

    svs, dvs = 13, 24
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, svs, MC.HASH_MAX), MapDef(MAP_HASH, 4, dvs, MC.HASH_MAX))
    asrc = vm.add_map(MapDef(MAP_ARRAY, 4, svs, 10))
    adst = vm.add_map(MapDef(MAP_ARRAY, 4, dvs, 300))
    odd = vm.add_map(MapDef(MAP_HASH, 4, 12, 16))   # a value_size that is no multiple of 8
    nokey = vm.add_map(MapDef(MAP_HASH, 0, 16, 16))
    for d in (MapDef(MAP_ARRAY, 4, svs, 10), MapDef(MAP_ARRAY, 4, dvs, 300), MapDef(MAP_HASH, 4, 12, 16), MapDef(MAP_HASH, 0, 16, 16)):
        ref.add_map(d)
    SC.fill_hash(vm, ref, src, dev, rng, 8, svs, 30)
    install(vm, ref, dst, dev, hash_pool(rng, 4, 5), rng.integers(0, 256, size=(5, dvs), dtype=np.uint8))
    before = state_image(vm, src, dev), state_image(vm, dst, dev), state_image(vm, adst, dev)
    G, NONE = N.MapGroup, MG_NONE
    #            from off len moff mw  count sum pad
    bad = [(src, dst, None),                                   # g NULL
           (src, src, G(MG_KEY, 0, 8, 0, 0, 0, NONE, 0)),      # src == dst
           (src, dst, G(2, 0, 4, 0, 0, 0, NONE, 0)),           # from
           (src, dst, G(0xffffffff, 0, 4, 0, 0, 0, NONE, 0)),
           (src, dst, G(MG_KEY, 0, 4, 0, 0, 0, NONE, 1)),      # pad
           (src, dst, G(MG_KEY, 5, 4, 0, 0, 0, NONE, 0)),      # group bytes outside the 8-byte key
           (src, dst, G(MG_KEY, 0xfffffffe, 4, 0, 0, 0, NONE, 0)),
           (src, dst, G(MG_VALUE, svs - 3, 4, 0, 0, 0, NONE, 0)),  # ... outside the value
           (asrc, dst, G(MG_KEY, 1, 4, 0, 0, 0, NONE, 0)),     # ... outside an ARRAY source's four index bytes
           (src, dst, G(MG_KEY, 0, 3, 0, 0, 0, NONE, 0)),      # len != the destination's key_size
           (src, dst, G(MG_KEY, 0, 8, 0, 0, 0, NONE, 0)),
           (src, adst, G(MG_KEY, 0, 3, 0, 0, 0, NONE, 0)),     # ARRAY destination: len 1, 2 or 4
           (src, adst, G(MG_KEY, 0, 0, 0, 0, 0, NONE, 0)),
           (src, adst, G(MG_KEY, 0, 8, 0, 0, 0, NONE, 0)),
           (src, nokey, G(MG_KEY, 0, 0, 0, 0, 0, NONE, 0)),    # a HASH destination without key bytes
           (src, dst, G(MG_KEY, 0, 4, 0, 8, NONE, NONE, 0)),   # no accumulator
           (src, dst, G(MG_KEY, 0, 4, 0, 0, 0, 8, 0)),         # a sum without a measure
           (src, dst, G(MG_KEY, 0, 4, 0, 3, 0, 8, 0)),         # measure width
           (src, dst, G(MG_KEY, 0, 4, 0, 16, 0, 8, 0)),
           (src, dst, G(MG_KEY, 0, 4, svs - 7, 8, 0, 8, 0)),   # a measure outside the source value
           (src, dst, G(MG_KEY, 0, 4, 0xfffffffc, 4, 0, 8, 0)),
           (src, dst, G(MG_KEY, 0, 4, 0, 8, 4, NONE, 0)),      # an accumulator not 8-byte aligned
           (src, dst, G(MG_KEY, 0, 4, 0, 8, 0, 12, 0)),
           (src, dst, G(MG_KEY, 0, 4, 0, 8, dvs, NONE, 0)),    # ... not inside the destination value
           (src, dst, G(MG_KEY, 0, 4, 0, 8, 0, 0xfffffff8, 0)),
           (src, dst, G(MG_KEY, 0, 4, 0, 8, 8, 8, 0)),         # the accumulators overlap
           (src, odd, G(MG_KEY, 0, 4, 0, 8, 0, NONE, 0))]      # a destination value_size that is no multiple of 8
    for s, d, g in bad:
        what = None if g is None else tuple(getattr(g, f[0]) for f in g._fields_)
        assert raw_group(lib, vm, s, None, g, d)[0] == MC.ERR_INVAL, (s, d, what)
    ok = G(MG_KEY, 0, 4, 0, 8, 0, 8, 0)
    assert raw_group(lib, vm, src, None, ok, dst, matched=False)[0] == MC.ERR_INVAL  # a NULL matched
    for f in (N.MapFilter(9, 0, 1, 0, 0), N.MapFilter(EQ, 0, 1, 1, 0), N.MapFilter(EQ, 0, 3, 0, 0), N.MapFilter(EQ, svs, 1, 0, 0)):
        assert raw_group(lib, vm, src, f, ok, dst)[0] == MC.ERR_INVAL  # the scan's filter errors
    assert raw_group(lib, vm, 99, None, ok, dst)[0] == MC.ERR_INVAL  # a bad map index
    assert raw_group(lib, vm, src, None, ok, 99)[0] == MC.ERR_INVAL
    after = state_image(vm, src, dev), state_image(vm, dst, dev), state_image(vm, adst, dev)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused call changed a map"
    same_map(vm, ref, src, "after the refused calls")
    same_dst(vm, ref, dst, dev, "after the refused calls")
    # a NULL created is allowed
    rc, matched, _ = raw_group(lib, vm, src, None, ok, dst, created=False)
    assert (rc, matched) == (0, 20)
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 13. the Python interface
def run_python_api(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(1313)
    vm, ref, src, dst = two_maps(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, MC.HASH_MAX), MapDef(MAP_ARRAY, 4, 16, 256))
    SC.fill_hash(vm, ref, src, dev, rng, 8, 16, 40, delete_third=False)
    snap = Snapshot(vm, ref, src, dev)
    g = MapGroup(MG_VALUE, 2, 1, count_off=8, sum_off=0, measure_off=4, measure_width=4)
    flt = MapFilter(ANYBITS, 0, 1, 0x3f)
    sel = selects(snap.vals, flt)
    groups = expect_groups(snap.keys[sel], snap.vals[sel], g)
    assert vm.map_group(src, dst, g, flt) == (int(sel.sum()), 0)
    oracle_fold(ref, dst, groups, g)
    same_dst(vm, ref, dst, dev, "VM.map_group")
    hdst = vm.add_map(MapDef(MAP_HASH, 1, 16, 256))
    ref.add_map(MapDef(MAP_HASH, 1, 16, 256))
    assert vm.map_group(src, hdst, g) == (40, len(expect_groups(snap.keys, snap.vals, g)))
    oracle_fold(ref, hdst, expect_groups(snap.keys, snap.vals, g), g)
    same_dst(vm, ref, hdst, dev, "VM.map_group into a HASH map")
    vm.close()
    ref.close()
