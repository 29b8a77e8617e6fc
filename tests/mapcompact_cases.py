"""Shared cases of the device-side tombstone compaction (xe_map_compact): tests/test_mapcompact.py runs them on
the host simulation, tests/test_mapcompact_gpu.py on the product library.

No expected value comes from the code under test. The yardstick is expect_compact, a restatement of the call's
definition (include/xdpemu.h) over the image exported before the call (xe_map_state_export, device to device:
the tombstones are in it): every run of non-free records that holds a tombstone is cleared and its entries are
inserted again in run order, each by a linear probe from its home slot. It is a full rebuild with scratch, not
the kernels' in-place walk. It yields the whole image after the call and the call's info; every case compares all
bytes and all four numbers. What a host visit leaves (HostMap::drop_tombstones: the whole table cleared, the
entries inserted again from slot 0) is restated beside it: where the two layouts are the same bytes, which the
cases without a wrapping run assert, a second VM of the same library that imported the same image and made one
host visit must hold exactly the compacted image. (A run WITHOUT a tombstone that wraps the table's end is
left alone by the call, while a host visit may arrange it differently; so the comparison is made where the two
restatements agree, not merely where no run with a tombstone wraps.) Every case also agrees with the oracle, at
whose interface a compaction is invisible: same_image_map without a host visit, same_map with one.

Each case asserts from the model that what it is meant to reach occurs (entries move, a run wraps, a run crosses
a tile edge): another seed cannot turn it into a no-op silently.

Sizes (xe_mapops.h / xe_mapops.hip): a tile is 256 slots in 4 rounds of 64 lanes, one bitmap word a round; tables
below 64 slots keep the wrap predecessor inside word 0; values of up to 16 bytes move on the run's own lane,
larger ones by the whole wave (in units of 16, 8, 4 or 1 bytes); records have 2, 4, 8 or 16 words; a run with a
tombstone that is longer than kMcMaxRun slots goes through the host."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np

import mapops_cases as MC
import mapscan_cases as SC
from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY, MAP_QUEUE, MAP_STACK, VM, MapDef, MapFilter,
                                  Settings)
from mapgroup_cases import install, remove
from mapops_cases import (GUARD, SLOT_FULL, SLOT_TOMB, SLOT_VLEN0, Runner, addr, flow_vm, hash_geometry, home_slot, image_records,
                          keys_with_home, pair, same_image_map, same_map, settle, state_image, to_np)

COUNT_ONLY = 1  # XE_MC_COUNT_ONLY
KEY_SIZES = (4, 8, 13, 24, 56, 64)                  # every record size: 2, 2, 4, 4, 8 and 16 words
VALUE_SIZES = (1, 8, 16, 17, 64, 65, 1025, 4096)    # the lane-alone path, every mo_move unit, the wave path
MAX_RUN = int(re.search(r"kMcMaxRun = (\d+)", (Path(__file__).resolve().parent.parent / "gobpfld_amd" / "csrc" / "xe_mapops.h").read_text()).group(1))


# ---------------------------------------------------------------- the definition, restated
def views(vm: VM, m: int, img: np.ndarray):
    """(records [cap + 1, words] as u64, values [cap + 1, value_size]) of a HASH image, as views into it."""
    cap, rw, vals_alloc = hash_geometry(vm, m)
    vs = vm.map_defs[m].value_size
    return img[vals_alloc:vals_alloc + (cap + 1) * rw * 8].view(np.uint64).reshape(cap + 1, rw), img[:(cap + 1) * vs].reshape(cap + 1, vs)


def rebuild(rec: np.ndarray, vals: np.ndarray, cap: int, ks: int, slots) -> int:
    """Clears `slots` and inserts their entries again in that order, each by a linear probe from its home slot.
    Returns the entries that changed slot."""
    full = [(int(s), rec[s].copy(), vals[s].copy()) for s in slots if int(rec[s, 0]) & SLOT_FULL]
    rec[slots] = 0
    vals[slots] = 0
    moved = 0
    for s, r, v in full:
        at = home_slot(r[1:].tobytes()[:ks], cap)
        while int(rec[at, 0]) & SLOT_FULL:
            at = (at + 1) & (cap - 1)
        rec[at], vals[at] = r, v
        rec[at, 0] = int(r[0]) & (SLOT_FULL | SLOT_VLEN0)
        moved += at != s
    return moved


def expect_compact(vm: VM, m: int, img: np.ndarray, max_run: int = MAX_RUN, with_host: bool = True) -> dict:
    """What xe_map_compact must report and leave, given the image before it: `image`; `info` = (tombstones,
    moved, longest_run, via_host); `host_image`: what a host visit leaves instead; `wraps`: a rebuilt run passes
    the table's end; `runs`: (first slot, slots) of every run that holds a tombstone. with_host False: no `host_image`
    (a profile's table of 2^21 slots)."""
    cap = hash_geometry(vm, m)[0]
    ks = vm.map_defs[m].key_size
    out, host = img.copy(), img.copy()
    rec, vals = views(vm, m, out)
    w0 = rec[:cap, 0].copy()
    free, tomb = (w0 & np.uint64(SLOT_FULL | SLOT_TOMB)) == 0, (w0 & np.uint64(SLOT_FULL | SLOT_TOMB)) == np.uint64(SLOT_TOMB)
    tombs, moved, longest, wraps, long, runs = int(tomb.sum()), 0, 0, False, False, []
    if tombs and (with_host or not free.any()):
        rebuild(*views(vm, m, host), cap, ks, np.arange(cap))
    if tombs and not free.any():  # no run has a start: through the host
        return dict(image=host, info=(tombs, 0, cap, 1), host_image=host, wraps=False, runs=[(0, cap)])
    for s in np.nonzero(~free & np.roll(free, 1))[0] if tombs else ():
        n = 1
        while not free[(s + n) % cap]:
            n += 1
        slots = (int(s) + np.arange(n)) % cap
        if not tomb[slots].any():
            continue
        runs.append((int(s), n))
        longest = max(longest, n)
        if n > max_run:
            long = True
            continue
        wraps |= int(s) + n > cap
        moved += rebuild(rec, vals, cap, ks, slots)
    if long:  # the partly compacted table goes through the host
        rebuild(rec, vals, cap, ks, np.arange(cap))
        moved = 0
    return dict(image=out, info=(tombs, moved, longest, int(long)), host_image=host, wraps=wraps, runs=runs)


# ---------------------------------------------------------------- the call and its check
def raw_compact(lib, vm: VM, m: int, flags: int = 0, with_info: bool = True):
    """One call. Returns (rc, (tombstones, moved, longest_run, via_host))."""
    info = N.MapCompactInfo(0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF)
    rc = lib.map_compact(vm.h, m, flags, C.byref(info) if with_info else None, None)
    return rc, (info.tombstones, info.moved, info.longest_run, info.via_host)


def host_visit_image(lib, vm: VM, m: int, dev, img: np.ndarray) -> np.ndarray:
    """The image of a second VM of the same library that imported `img` and then made one host visit
    (map_dump; the export is the device call that uploads the rebuilt mirror)."""
    twin = VM(Settings(engine=1), lib=lib)
    for i in range(1, m + 1):
        assert twin.add_map(vm.map_defs[i]) == i
    buf = dev(img)
    settle(buf)
    twin.map_state_import(m, addr(buf))
    twin.map_dump(m)
    out = state_image(twin, m, dev)
    twin.close()
    return out


def check_compact(lib, vm: VM, ref: VM, m: int, dev, what: str, twin: bool = True, count_first: bool = True) -> dict:
    """A COUNT_ONLY call, then the real one, against the model of the image before them; the second VM where
    the model says the host's layout is the same; the oracle without a host visit. Returns the model."""
    before = state_image(vm, m, dev)
    exp = expect_compact(vm, m, before)
    tombs, moved, longest, via_host = exp["info"]
    traffic = vm.map_traffic(m)
    if count_first:
        rc, info = raw_compact(lib, vm, m, COUNT_ONLY)
        assert rc == 0, f"{what}: {lib.last_error(vm.h)}"
        assert info == (tombs, 0, longest, 0), f"{what}: COUNT_ONLY reports {info}, expected {(tombs, 0, longest, 0)}"
        assert np.array_equal(before, state_image(vm, m, dev)), f"{what}: COUNT_ONLY changed the map"
        assert vm.map_traffic(m) == traffic, f"{what}: COUNT_ONLY moved the whole map"
    rc, info = raw_compact(lib, vm, m)
    assert rc == 0, f"{what}: {lib.last_error(vm.h)}"
    assert info == exp["info"], f"{what}: info {info}, expected {exp['info']}"
    assert vm.map_traffic(m) == (traffic[0] + via_host, traffic[1] + via_host), f"{what}: whole-map transfers {vm.map_traffic(m)} after {traffic}"
    after = state_image(vm, m, dev)
    diff = np.nonzero(after != exp["image"])[0]
    assert not len(diff), f"{what}: {len(diff)} bytes of the image differ from the model, the first at {int(diff[0])}"
    w0 = image_records(vm, m, after)[0]
    assert not (w0[:-1] & np.uint64(SLOT_TOMB)).any(), f"{what}: a tombstone is left"
    assert after[-8:].tobytes() == before[-8:].tobytes(), f"{what}: the count changed"
    if twin and np.array_equal(exp["image"], exp["host_image"]):
        assert np.array_equal(after, host_visit_image(lib, vm, m, dev, before)), f"{what}: a host visit leaves another image"
        exp["twin"] = True
    same_image_map(vm, ref, m, dev, what)
    assert raw_compact(lib, vm, m) == (0, (0, 0, 0, 0)), f"{what}: a second compaction found something to do"
    assert np.array_equal(after, state_image(vm, m, dev)), f"{what}: a second compaction changed the map"
    return exp


def keys_at(cap: int, homes, start: int = 1) -> np.ndarray:
    """One distinct 8-byte key (a counter) per element of `homes`, with that home slot in a table of cap slots."""
    c = np.arange(start, start + 32 * cap + 4096, dtype=np.uint64)
    home = ((SC.hash8(c) & np.uint64(0xffffffff)) & np.uint64(cap - 1)).astype(np.int64)
    order = np.argsort(home, kind="stable")
    first = np.searchsorted(home[order], np.arange(cap))
    used: dict[int, int] = {}
    out = []
    for h in homes:
        i = first[h] + used.get(h, 0)
        used[h] = used.get(h, 0) + 1
        assert i < len(c) and home[order[i]] == h, "not enough candidate keys"
        out.append(c[order[i]])
    keys = np.ascontiguousarray(np.array(out, dtype=np.uint64).view(np.uint8).reshape(-1, 8))
    for k, h in list(zip(keys, homes))[:3]:  # the vectorised hash is the restated one
        assert home_slot(k.tobytes(), cap) == h
    return keys


def fill(vm: VM, ref: VM, m: int, dev, rng, ks: int, vs: int) -> None:
    """60 entries in the 128 slots of a HASH_MAX map, a third of them deleted again through map_delete_batch:
    twelve keys whose homes are four neighbouring slots, one a call (their order is then the same on every
    library), so that entries behind the deleted ones are sure to move; then 48 random ones."""
    chain = np.frombuffer(b"".join(keys_with_home(ks, range(40, 44), 12)), dtype=np.uint8).reshape(-1, ks)
    for k in chain:
        install(vm, ref, m, dev, k[None, :], rng.integers(0, 256, size=(1, vs), dtype=np.uint8))
    keys = MC.hash_pool(rng, ks, 48)
    install(vm, ref, m, dev, keys, rng.integers(0, 256, size=(48, vs), dtype=np.uint8))
    remove(vm, ref, m, dev, np.concatenate([chain[::3], keys[::3]]))


# ---------------------------------------------------------------- 1. matrix
def run_matrix(lib, oracle_lib, dev, ks: int, vs: int) -> None:
    rng = np.random.default_rng(100 * ks + vs)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    assert hash_geometry(vm, m)[0] == MC.HASH_CAP
    fill(vm, ref, m, dev, rng, ks, vs)
    exp = check_compact(lib, vm, ref, m, dev, f"keys of {ks}, values of {vs} bytes")
    assert exp["info"][0] == 20 and exp["info"][1] > 0 and exp["info"][3] == 0, exp["info"]
    assert exp["wraps"] or exp.get("twin"), "a table without a wrapping run was not compared with a host visit"
    same_map(vm, ref, m, f"keys of {ks}, values of {vs} bytes")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 2. geometry
# A run placed by hand: (first slot, the home of each entry as an offset into the run, the entries deleted again).
# Entry i is installed alone, after entries 0 .. i - 1, and its home offset is at most i: it lands at offset i.
GEOMETRY = ("wrap_high", "wrap_low", "start0")
GEOMETRY_TABLES = (8, 32, 33, 256)  # max_entries: 16, 64, 128 and 512 slots


def geometry_runs(cap: int, which: str):
    if which == "wrap_high":    # slots cap - 2, cap - 1, 0, 1 with the tombstone in slot cap - 1
        runs = [(cap - 2, (0, 0, 1, 2), (1,))]
    elif which == "wrap_low":   # ... with the tombstone in slot 0
        runs = [(cap - 2, (0, 0, 1, 2), (2,))]
    else:                       # a run that starts at slot 0 while slot cap - 1 is free
        runs = [(0, (0, 0, 0), (0,))]
    runs.append((5, (0, 0), (0,)))   # a tombstone as the first record of its run
    runs.append((9, (0, 0), (1,)))   # ... as the last
    if cap >= 128:
        runs.append((61, (0, 0, 1, 1, 3), (1,)))    # across slot 63 -> 64: the next word of the bitmaps
    if cap >= 512:
        runs.append((253, (0, 0, 1, 1, 3), (2,)))   # across slot 255 -> 256: the next tile
    return runs


def build_runs(vm: VM, ref: VM, m: int, dev, cap: int, runs, vs: int, rng) -> None:
    dead = []
    for start, hoffs, gone in runs:
        keys = keys_at(cap, [(start + h) % cap for h in hoffs], start=1 + 100000 * len(dead))
        vals = rng.integers(1, 256, size=(len(keys), vs), dtype=np.uint8)
        for i in range(len(keys)):
            install(vm, ref, m, dev, keys[i:i + 1], vals[i:i + 1])
        dead.append(keys[list(gone)])
    remove(vm, ref, m, dev, np.concatenate(dead))
    w0 = image_records(vm, m, state_image(vm, m, dev))[0]
    for start, hoffs, gone in runs:  # the layout is the one meant
        for i in range(len(hoffs)):
            assert int(w0[(start + i) % cap]) == (SLOT_TOMB if i in gone else SLOT_FULL), (start, i, int(w0[(start + i) % cap]))
        assert int(w0[(start - 1) % cap]) == 0 and int(w0[(start + len(hoffs)) % cap]) == 0


def run_geometry(lib, oracle_lib, dev, max_entries: int, which: str, vs: int) -> None:
    rng = np.random.default_rng(max_entries)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, vs, max_entries))
    cap = hash_geometry(vm, m)[0]
    assert cap == {8: 16, 32: 64, 33: 128, 256: 512}[max_entries]
    runs = geometry_runs(cap, which)
    build_runs(vm, ref, m, dev, cap, runs, vs, rng)
    exp = check_compact(lib, vm, ref, m, dev, f"{which} in {cap} slots")
    assert sorted(exp["runs"]) == sorted((s, len(h)) for s, h, _ in runs)
    assert exp["wraps"] == (which != "start0")
    # wrap_high: offsets 2 and 3 move up; wrap_low: offset 3; start0: offsets 1 and 2; the run with its tombstone
    # first: one entry; the runs across a word and a tile edge: the entries behind the tombstone
    want = {"wrap_high": 2, "wrap_low": 1, "start0": 2}[which] + 1 + (3 if cap >= 128 else 0) + (2 if cap >= 512 else 0)
    assert exp["info"] == (len(runs), want, 5 if cap >= 128 else 4 if which != "start0" else 3, 0), exp["info"]
    assert which != "start0" or exp.get("twin"), "a table without a wrapping run was not compared with a host visit"
    same_map(vm, ref, m, f"{which} in {cap} slots")
    vm.close()
    ref.close()


def run_only_tombstones(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(21)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 13, 24, MC.HASH_MAX))
    keys = MC.hash_pool(rng, 13, 40)
    install(vm, ref, m, dev, keys, rng.integers(1, 256, size=(40, 24), dtype=np.uint8))
    remove(vm, ref, m, dev, keys)
    exp = check_compact(lib, vm, ref, m, dev, "tombstones only")
    assert exp["info"][:2] == (40, 0) and exp.get("twin")
    assert not state_image(vm, m, dev).any(), "a table of tombstones did not become all zero"
    assert vm.map_count(m) == ref.map_count(m) == 0
    vm.close()
    ref.close()


def run_no_tombstones(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(22)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 24, MC.HASH_MAX))
    SC.fill_hash(vm, ref, m, dev, rng, 8, 24, 60, delete_third=False)
    before = state_image(vm, m, dev)
    exp = check_compact(lib, vm, ref, m, dev, "no tombstones")
    assert exp["info"] == (0, 0, 0, 0)
    assert np.array_equal(before, state_image(vm, m, dev)), "a compaction of nothing changed the map"
    empty = vm.add_map(MapDef(MAP_HASH, 8, 8, 16))
    assert ref.add_map(MapDef(MAP_HASH, 8, 8, 16)) == empty
    assert check_compact(lib, vm, ref, empty, dev, "an empty map")["info"] == (0, 0, 0, 0)
    same_map(vm, ref, m, "no tombstones")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 3. long runs
LONG_MAX, LONG_CAP, LONG_START = 8192, 16384, 1000


def run_long(lib, oracle_lib, dev, slots: int, vs: int = 8) -> None:
    """One run of exactly `slots` slots: the first entry at home, every other one slot behind its home, so
    that the tombstone made of the second entry lets every entry behind it move up by one."""
    rng = np.random.default_rng(slots)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, vs, LONG_MAX))
    assert hash_geometry(vm, m)[0] == LONG_CAP and slots <= LONG_MAX
    keys = keys_at(LONG_CAP, [LONG_START] + [LONG_START + j - 1 for j in range(1, slots)])
    vals = rng.integers(1, 256, size=(slots, vs), dtype=np.uint8)
    # The layout that installing the keys one after another and deleting the second leaves, written into an image
    # and imported (4,096 single calls would take seconds; the claims of one launch race for the slots).
    img = state_image(vm, m, dev)
    assert not img.any()
    rec, ivals = views(vm, m, img)
    at = LONG_START + np.arange(slots)
    rec[at, 0], rec[at, 1], ivals[at] = SLOT_FULL, keys.view(np.uint64).reshape(-1), vals
    rec[at[1], 0], ivals[at[1]] = SLOT_TOMB, 0
    img[-8:-4] = np.array([slots - 1], dtype=np.uint32).view(np.uint8)
    buf = dev(img)
    settle(buf)
    vm.map_state_import(m, addr(buf))
    live = np.ones(slots, dtype=bool)
    live[1] = False
    MC.ref_update(ref, m, keys[live], vals[live])
    same_image_map(vm, ref, m, dev, f"the imported run of {slots} slots")
    exp = check_compact(lib, vm, ref, m, dev, f"a run of {slots} slots")
    assert exp["runs"] == [(LONG_START, slots)], exp["runs"]
    via_host = int(slots > MAX_RUN)
    assert exp["info"] == (1, 0 if via_host else slots - 2, slots, via_host), exp["info"]
    same_map(vm, ref, m, f"a run of {slots} slots")
    vm.close()
    ref.close()


def run_no_free_record(lib, oracle_lib, dev) -> None:
    """The table of mapops_cases.run_tombstone_churn, taken to the end: three entries and 125 tombstones in
    128 slots, no free record."""
    rng = np.random.default_rng(11)
    ks, vs = 8, 8
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, ks, vs, MC.HASH_MAX))
    pool = MC.hash_pool(rng, ks, 4 * MC.HASH_MAX)
    install(vm, ref, m, dev, pool[:3], rng.integers(1, 256, size=(3, vs), dtype=np.uint8))
    for keys in (pool[64:125], pool[128:189], pool[192:195]):
        install(vm, ref, m, dev, keys, rng.integers(1, 256, size=(len(keys), vs), dtype=np.uint8))
        remove(vm, ref, m, dev, keys)
    w0 = image_records(vm, m, state_image(vm, m, dev))[0][:-1]
    assert int((w0 == np.uint64(SLOT_TOMB)).sum()) == 125 and int((w0 == np.uint64(SLOT_FULL)).sum()) == 3
    exp = check_compact(lib, vm, ref, m, dev, "no free record")
    assert exp["info"] == (125, 0, MC.HASH_CAP, 1)
    same_map(vm, ref, m, "no free record")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 4. flags and kinds
def run_flags_and_kinds(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(41)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, MC.HASH_MAX))
    fill(vm, ref, m, dev, rng, 8, 16)
    before = state_image(vm, m, dev)
    exp = expect_compact(vm, m, before)
    assert exp["info"][1] > 0
    for flags in (2, 3, 0x80000000, 0xfffffffe):
        assert raw_compact(lib, vm, m, flags)[0] == MC.ERR_INVAL, flags
    for flags in (0, COUNT_ONLY):
        assert raw_compact(lib, vm, m, flags, with_info=False)[0] == MC.ERR_INVAL
        assert raw_compact(lib, vm, 99, flags)[0] == MC.ERR_INVAL  # a bad map index
    assert np.array_equal(before, state_image(vm, m, dev)), "a refused call changed the map"
    # COUNT_ONLY and the real call after it report the same tombstones and longest run
    _, counted = raw_compact(lib, vm, m, COUNT_ONLY)
    _, real = raw_compact(lib, vm, m)
    assert (counted[0], counted[2]) == (real[0], real[2]) == (exp["info"][0], exp["info"][2]) and real == exp["info"]
    assert np.array_equal(state_image(vm, m, dev), exp["image"])
    same_map(vm, ref, m, "after COUNT_ONLY and the real call")
    # an ARRAY: zeros
    arr = vm.add_map(MapDef(MAP_ARRAY, 4, 8, 10))
    vm.map_update(arr, (3).to_bytes(4, "little"), b"\x07" * 8)
    for flags in (0, COUNT_ONLY):
        assert raw_compact(lib, vm, arr, flags) == (0, (0, 0, 0, 0))
    assert vm.map_lookup(arr, (3).to_bytes(4, "little")) == b"\x07" * 8
    vm.close()
    ref.close()
    # under an open epoch (a VM with a program): COUNT_ONLY alone
    vm, m = flow_vm(lib)
    keys, vals = MC.flow_entries(range(64))
    vm.map_update_batch_device(m, dev(keys), dev(vals))
    assert to_np(vm.map_delete_batch(m, dev(keys[::2].copy()))).all()
    before = state_image(vm, m, dev)
    exp = expect_compact(vm, m, before)
    assert exp["info"][0] == 32
    vm.epoch_begin()
    assert raw_compact(lib, vm, m)[0] == MC.ERR_INVAL
    assert raw_compact(lib, vm, m, COUNT_ONLY) == (0, (32, 0, exp["info"][2], 0))
    assert np.array_equal(before, state_image(vm, m, dev)), "a call under an open epoch changed the map"
    vm.epoch_end()
    assert raw_compact(lib, vm, m) == (0, exp["info"])
    assert np.array_equal(state_image(vm, m, dev), exp["image"])
    vm.close()
    for t in (MAP_LRU_HASH, MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY):
        vm = VM(Settings(engine=1), lib=lib)
        bad = vm.add_map(MapDef(t, 4, 16, 16) if t in (MAP_LRU_HASH, MAP_PERF_EVENT_ARRAY) else MapDef(t, 0, 16, 16))
        for flags in (0, COUNT_ONLY):
            assert raw_compact(lib, vm, bad, flags)[0] == MC.ERR_UNSUPPORTED, (t, flags)
            assert b"ARRAY and HASH" in lib.last_error(vm.h)
        vm.close()


# ---------------------------------------------------------------- 5. nil-backed values, the empty key
def keys4_at(cap: int, home: int, skip) -> bytes:
    """A 4-byte key (a counter from 1000 on) with the given home slot that is none of `skip`."""
    i = 1000
    while home_slot(i.to_bytes(4, "little"), cap) != home or i.to_bytes(4, "little") in skip:
        i += 1
    return i.to_bytes(4, "little")


def run_vlen0(lib, oracle_lib, dev) -> None:
    """mapops_cases.run_vlen0's batch leaves three of the keys 0 .. 3 nil-backed. Every key's home slot is
    taken by another key first, which is deleted after the batch: the nil-backed records move."""
    from parity import packets
    from test_lru_nil_value import _program
    umem, descs = packets(600, 64, seed=9)
    for d in descs:
        umem[int(d["addr"]) + 1] = 0
    for i in (150, 151, 400):
        umem[int(descs[i]["addr"]) + 1] = 1
    keys = np.array([0, 1, 2, 3], dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    vms = []
    for lb in (lib, oracle_lib):
        vm = VM(Settings(engine=1), lib=lb)
        m = vm.add_map(MapDef(MAP_HASH, 4, 8, 16))
        vm.set_entrypoint(vm.add_raw_program(_program()))
        vms.append(vm)
    vm, ref = vms
    cap = hash_geometry(vm, m)[0]
    blockers, skip = [], {k.tobytes() for k in keys}
    for h in sorted({home_slot(k.tobytes(), cap) for k in keys}):
        blockers.append(keys4_at(cap, h, skip))
        skip.add(blockers[-1])
    blockers = np.frombuffer(b"".join(blockers), dtype=np.uint8).reshape(-1, 4)
    for v in vms:
        for b in blockers:
            v.map_update(m, b.tobytes(), b"\x99" * 8)
    got, want = vm.run_batch(umem.copy(), descs), ref.run_batch(umem.copy(), descs)
    assert np.array_equal(got.verdicts, want.verdicts)
    remove(vm, ref, m, dev, blockers)
    before = state_image(vm, m, dev)
    w0, ikeys, _, _ = image_records(vm, m, before)
    nil = {ikeys[s].tobytes(): s for s in np.nonzero(w0 & np.uint64(SLOT_VLEN0))[0]}
    assert len(nil) == 3, "the batch left no nil-backed records on the device"
    exp = check_compact(lib, vm, ref, m, dev, "nil-backed records")
    w1, keys1, vals1, _ = image_records(vm, m, exp["image"])
    now = {keys1[s].tobytes(): s for s in np.nonzero(w1 & np.uint64(SLOT_VLEN0))[0]}
    assert set(now) == set(nil) and all(int(w1[s]) == (SLOT_FULL | SLOT_VLEN0) for s in now.values())
    assert any(now[k] != nil[k] for k in nil), "no nil-backed record moved"
    MC.check_lookup(vm, ref, m, np.ascontiguousarray(np.concatenate([keys, blockers])), 8, dev, "lookups after moving nil-backed records")
    same_map(vm, ref, m, "nil-backed records")
    vm.close()
    ref.close()


def run_empty_key(lib, oracle_lib, dev) -> None:
    """A HASH map with key_size 0 keeps its one entry in the record past the table, which no compaction
    touches: as an entry, and as the tombstone a device delete leaves there."""
    vs = 24
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 0, vs, MC.HASH_MAX))
    other = vm.add_map(MapDef(MAP_HASH, 8, vs, MC.HASH_MAX))  # a map that holds entries beside it
    assert ref.add_map(MapDef(MAP_HASH, 8, vs, MC.HASH_MAX)) == other
    fill(vm, ref, other, dev, np.random.default_rng(51), 8, vs)
    for v in (vm, ref):
        v.map_update(m, b"", b"\x31" * vs)
    cap = hash_geometry(vm, m)[0]
    w0, _, vals, count = image_records(vm, m, state_image(vm, m, dev))
    assert int(w0[cap]) == SLOT_FULL and count == 1 and vals[cap].tobytes() == b"\x31" * vs
    assert check_compact(lib, vm, ref, m, dev, "the empty key")["info"] == (0, 0, 0, 0)
    assert check_compact(lib, vm, ref, other, dev, "the map beside it")["info"][1] > 0
    assert vm.map_lookup(m, b"") == b"\x31" * vs
    some = dev(np.zeros(64, dtype=np.uint8))
    settle(some)
    if MC.on_dev(some):
        assert lib.map_delete_batch_device(vm.h, m, addr(some), 1, None, None) == 0
    else:
        assert lib.map_delete_batch(vm.h, m, addr(some), 1, None) == 0
    ref.map_delete(m, b"")
    before = state_image(vm, m, dev)
    assert int(image_records(vm, m, before)[0][cap]) == SLOT_TOMB
    assert raw_compact(lib, vm, m) == (0, (0, 0, 0, 0))  # the record past the table is no slot of the table
    assert np.array_equal(before, state_image(vm, m, dev))
    same_map(vm, ref, m, "the empty key deleted")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 6. the delta base
def key_deltas(vm: VM, m: int, dev) -> tuple[dict, np.ndarray, np.ndarray]:
    """({key: its value's delta since the batch}, the deltas of every slot, word 0 of every slot)."""
    out = dev(np.full(vm.map_values_bytes(m), GUARD, np.uint8))
    settle(out)
    vm.map_delta(m, addr(out), lane=8)
    w0, keys, _, _ = image_records(vm, m, state_image(vm, m, dev))
    delta = to_np(out)[:len(w0) * 16].reshape(-1, 16)
    full = np.nonzero(w0 & np.uint64(SLOT_FULL))[0]
    return {keys[s].tobytes(): delta[s].tobytes() for s in full}, delta, w0


def run_delta_base(lib, oracle_lib, dev) -> None:
    """mapscan_cases.run_traffic's setup: flows installed, one batch whose adds are in xe_map_delta, a device
    expire. The compaction moves values and their delta base together."""
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    r = Runner(vm, dev, False)
    keys, vals = MC.flow_entries(list(range(56)) + [(1 << 41) + i for i in range(600)])
    install(vm, ref, m, dev, keys, vals)
    r.run(0)  # the map is now newer on the device, and the batch's adds are its delta
    umem, descs = MC.W.build_batch("c3learn", 0, MC.FLOW_PACKETS)
    ref.run_batch(umem, descs)
    k, _, matched = vm.map_expire(m, MapFilter(SC.EQ, 8, 8, 0))  # the 600 flows no packet belongs to
    assert matched == 600
    MC.ref_delete(ref, rm, to_np(k))
    traffic = vm.map_traffic(m)
    before, _, _ = key_deltas(vm, m, dev)
    assert any(any(d) for d in before.values()), "the batch's adds are not in the delta"
    exp = check_compact(lib, vm, ref, m, dev, "a flow table with a delta", twin=False)
    assert exp["info"][0] == 600 and exp["info"][1] > 0 and exp["info"][3] == 0, exp["info"]
    after, delta, w0 = key_deltas(vm, m, dev)
    assert after == before, "a key's delta changed with the compaction"
    assert not delta[(w0 & np.uint64(SLOT_FULL)) == 0].any(), "a record that is no entry shows a delta"
    assert vm.map_traffic(m) == traffic, "the compaction moved the whole map"
    same_map(vm, ref, m, "a flow table with a delta")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 7. under traffic
def run_mixed(lib, oracle_lib, dev, use_async: bool) -> None:
    vm, m = flow_vm(lib)
    ref, rm = flow_vm(oracle_lib)
    r = Runner(vm, dev, use_async)
    keys, vals = MC.flow_entries(list(range(24)) + [(1 << 41) + i for i in range(300)])
    install(vm, ref, m, dev, keys, vals)

    def ref_run(start: int) -> np.ndarray:
        umem, descs = MC.W.build_batch("c3learn", start, MC.FLOW_PACKETS)
        return ref.run_batch(umem, descs).verdicts

    v0, w0 = r.run(0), ref_run(0)
    # no xe_sync in between: the expire completes the pipeline itself
    gone, _, matched = vm.map_expire(m, MapFilter(SC.ANYBITS, 0, 1, 1))  # every entry with an odd first value byte
    assert np.array_equal(to_np(v0), w0)
    rk, rv = ref.map_dump(rm)
    sel = SC.selects(rv, MapFilter(SC.ANYBITS, 0, 1, 1))
    gone = to_np(gone)
    assert matched == int(sel.sum()) > 100 and {bytes(x) for x in gone} == {bytes(x) for x in rk[sel]}
    MC.ref_delete(ref, rm, rk[sel])
    traffic = vm.map_traffic(m)
    exp = check_compact(lib, vm, ref, m, dev, "between two batches", twin=False)
    assert exp["info"][0] == matched and exp["info"][1] > 0 and exp["info"][3] == 0, exp["info"]
    assert vm.map_traffic(m) == traffic, "the compaction moved the whole map"
    v1, w1 = r.run(MC.FLOW_PACKETS), ref_run(MC.FLOW_PACKETS)  # the keyed path learns flows again
    nk, nv = MC.flow_entries([(1 << 42) + i for i in range(200)])
    install(vm, ref, m, dev, nk, nv)  # (completes the pipeline)
    assert np.array_equal(to_np(v1), w1)
    live = ref.map_dump(rm)[0]
    MC.check_lookup(vm, ref, m, np.ascontiguousarray(np.concatenate([live, gone, nk])), 16, dev, "every live key and the expired ones")
    assert vm.map_traffic(m) == traffic
    # a batch in flight when the compaction is called: it completes first
    v2 = r.run(2 * MC.FLOW_PACKETS)
    rc, info = raw_compact(lib, vm, m)
    w2 = ref_run(2 * MC.FLOW_PACKETS)
    assert rc == 0 and info[3] == 0 and np.array_equal(to_np(v2), w2)
    same_image_map(vm, ref, m, dev, "after a compaction behind a batch")
    same_map(vm, ref, m, "after three batches and two compactions")
    vm.close()
    ref.close()


# ---------------------------------------------------------------- 8. determinism
def run_determinism(lib, oracle_lib, dev) -> None:
    """Two VMs that took the same calls, one entry a call, hold identical images after the compaction: a table
    with a wrapping run whose host layout is another one."""
    images = []
    for _ in range(2):
        rng = np.random.default_rng(81)
        vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 24, 32))
        # slots 62, 63, 0, 1, 2: the entry in slot 1 has its home in slot 63 and takes the tombstone's place in
        # slot 0, where a host visit puts the entry from slot 2 (it comes first from slot 0 on)
        build_runs(vm, ref, m, dev, 64, [(62, (0, 0, 1, 1, 2), (2,)), (20, (0, 0, 0, 1), (1,))], 24, rng)
        exp = check_compact(lib, vm, ref, m, dev, "a wrapping run")
        assert exp["wraps"] and exp["info"] == (2, 4, 5, 0), exp["info"]
        assert not np.array_equal(exp["image"], exp["host_image"]), "the host's layout of this wrapping run is the same one"
        images.append(state_image(vm, m, dev))
        same_map(vm, ref, m, "a wrapping run")
        vm.close()
        ref.close()
    assert np.array_equal(images[0], images[1])


# ---------------------------------------------------------------- 9. the Python interface
def run_python_api(lib, oracle_lib, dev) -> None:
    rng = np.random.default_rng(91)
    vm, ref, m, _ = pair(lib, oracle_lib, MapDef(MAP_HASH, 8, 16, MC.HASH_MAX))
    fill(vm, ref, m, dev, rng, 8, 16)
    tombs, moved, longest, _ = expect_compact(vm, m, state_image(vm, m, dev))["info"]
    assert vm.map_compact(m, count_only=True) == {"tombstones": tombs, "moved": 0, "longest_run": longest, "via_host": 0}
    assert vm.map_compact(m) == {"tombstones": tombs, "moved": moved, "longest_run": longest, "via_host": 0}
    assert vm.map_compact(m) == {"tombstones": 0, "moved": 0, "longest_run": 0, "via_host": 0}
    same_map(vm, ref, m, "VM.map_compact")
    vm.close()
    ref.close()
