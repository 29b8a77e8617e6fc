"""The refusals of the device-side map calls, as a table: every xe_map_*_batch / scan / top / stats / group / join /
compact / modify entry point and every xe_lru_* entry point, device form and host-pointer form, with the return code
AND the xe_last_error text of each refusal, on maps of 16 entries (the run_errors / run_limits cases of the
*_cases.py files check mostly the codes).

A row is (call, arguments, rc, text, uploads). The arguments name the row's maps and buffers by the letters below; a
leading "epoch" opens a shard epoch first. Every row runs on a VM of its own whose maps are host-dirty, so `uploads`
(xe_debug_map_traffic of the maps the row names, in the order it names them) says whether the refusal came before or
after the call had made the map current on the device: where a check stands among the others is part of what the
table pins, and the rows under "two refusals at once" pin which one wins. A refusal launches nothing, so the twin on
the product library (gpu) runs the same table in about a second; the few rows that are served, not refused (reads
during an epoch), do launch, so there the buffers of a _device call are device memory.

The expected values were recorded from the library before its host layer was consolidated."""
import ctypes as C

import numpy as np
import pytest

from gobpfld_amd import _native as N
from gobpfld_amd.emulator import (ENGINE_INTERP, MAP_ARRAY, MAP_HASH, MAP_LRU_HASH, MAP_QUEUE, VM, MapDef, Settings)

OK, INVAL, UNSUPPORTED = 0, -22, -95  # include/xdpemu.h XE_ERR_*
NONE = 0xffffffff  # XE_MG_NONE
BIG = (1 << 31) + 1
# the maps of a row's VM, 16 entries each: (type, key_size, value_size)
MAPS = {"A": (MAP_ARRAY, 4, 8), "H": (MAP_HASH, 4, 8), "L": (MAP_LRU_HASH, 4, 8), "Q": (MAP_QUEUE, 0, 8),
        "D": (MAP_HASH, 4, 16), "E": (MAP_HASH, 4, 12), "Z": (MAP_HASH, 0, 8), "B": (MAP_ARRAY, 4, 16)}
F, O, G, J, ED = N.MapFilter, N.MapOrder, N.MapGroup, N.MapJoin, N.MapEdit
ORD = O(0, 8, 0, 0)
GRP = G(0, 0, 4, 0, 8, 0, 8, 0)  # H's key groups into D: count at 0, sum of the u64 value at 8
JOIN = J(0, 0, 4, 0, 0, 0)  # H's key is looked up in D


def E(*edits):
    return (ED * max(len(edits), 1))(*edits)


ADD1 = E(ED(1, 0, 8, 0, 1))


def run_row(lib, call, args, device_buffer=None):
    """(rc, xe_last_error text or None after XE_OK, uploads of the maps named). device_buffer(nbytes): (an object that
    keeps zeroed device memory alive, its address), for the buffers of a _device call; None: host memory serves."""
    vm = VM(Settings(engine=ENGINE_INTERP), lib=lib)
    vm.set_entrypoint(vm.add_raw_program([0x2000000b7, 0x95]))  # r0 = 2; exit (xe_epoch_begin wants a program)
    idx = {}
    for name, (t, ks, vs) in MAPS.items():
        idx[name] = vm.add_map(MapDef(t, ks, vs, 16))
        if t != MAP_QUEUE:
            vm.map_update(idx[name], bytes(ks), bytes(vs))  # (host-dirty: the next device call uploads)
    if device_buffer is not None and call.endswith("_device"):
        bufs = {c: device_buffer(64) for c in "kvfj"}
    else:
        bufs = {c: (a, a.ctypes.data) for c, a in ((c, np.zeros(64, np.uint8)) for c in "kvfj")}
    outs = {c: C.c_uint64(7) for c in "nc"}
    outs["info"], outs["stats"] = N.MapCompactInfo(), N.MapStats()
    if args and args[0] == "epoch":
        vm.epoch_begin()
        args = args[1:]
    named, real = [], []
    for a in args:
        if isinstance(a, str) and a in idx:
            named.append(idx[a])
            real.append(idx[a])
        elif isinstance(a, str) and a in bufs:
            real.append(bufs[a][1])
        elif isinstance(a, str):
            real.append(C.byref(outs[a]))
        elif isinstance(a, C.Structure):
            real.append(C.byref(a))
        else:
            real.append(a)
    before = [vm.map_traffic(m)[0] for m in named]
    rc = getattr(lib, call)(vm.h, *real)
    text = None if rc == OK else lib.last_error(vm.h).decode()
    ups = tuple(vm.map_traffic(m)[0] - b for m, b in zip(named, before))
    vm.close()
    return rc, text, ups


ROWS = (
    # ---- map index out of bounds
    ("map_lookup_batch_device", (99, "k", 2, "v", "f", None), INVAL, 'map index out of bounds', ()),
    ("map_lookup_batch", (99, "k", 2, "v", "f"), INVAL, 'map index out of bounds', ()),
    ("map_update_batch_device", (99, "k", "v", 2, None), INVAL, 'map index out of bounds', ()),
    ("map_update_batch_staged", (99, "k", "v", 2), INVAL, 'map index out of bounds', ()),
    ("map_delete_batch_device", (99, "k", 2, "f", None), INVAL, 'map index out of bounds', ()),
    ("map_delete_batch", (99, "k", 2, "f"), INVAL, 'map index out of bounds', ()),
    ("map_modify_batch_device", (99, "k", 2, ADD1, 1, "v", "f", None), INVAL, 'map index out of bounds', ()),
    ("map_modify_batch", (99, "k", 2, ADD1, 1, "v", "f"), INVAL, 'map index out of bounds', ()),
    ("map_scan_device", (99, None, "k", "v", 2, "n", None), INVAL, 'map index out of bounds', ()),
    ("map_scan", (99, None, "k", "v", 2, "n"), INVAL, 'map index out of bounds', ()),
    ("map_expire_device", (99, None, "k", "v", 2, "n", None), INVAL, 'map index out of bounds', ()),
    ("map_expire", (99, None, "k", "v", 2, "n"), INVAL, 'map index out of bounds', ()),
    ("map_top_device", (99, None, ORD, "k", "v", 2, "n", "c", None), INVAL, 'map index out of bounds', ()),
    ("map_top", (99, None, ORD, "k", "v", 2, "n", "c"), INVAL, 'map index out of bounds', ()),
    ("map_evict_device", (99, None, ORD, "k", "v", 2, "n", "c", None), INVAL, 'map index out of bounds', ()),
    ("map_evict", (99, None, ORD, "k", "v", 2, "n", "c"), INVAL, 'map index out of bounds', ()),
    ("map_stats", (99, None, ORD, "stats", None), INVAL, 'map index out of bounds', ()),
    ("map_group", (99, None, GRP, "D", "n", "c", None), INVAL, 'map index out of bounds', (0,)),
    ("map_join_device", (99, None, JOIN, "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map index out of bounds', (0,)),
    ("map_join", (99, None, JOIN, "D", "k", "v", "j", 2, "n", "c"), INVAL, 'map index out of bounds', (0,)),
    ("map_compact", (99, 0, "info", None), INVAL, 'map index out of bounds', ()),
    ("map_modify_device", (99, None, ADD1, 1, "k", "v", 2, "n", None), INVAL, 'map index out of bounds', ()),
    ("map_modify", (99, None, ADD1, 1, "k", "v", 2, "n"), INVAL, 'map index out of bounds', ()),
    ("lru_lookup_batch_device", (99, "k", 2, "v", "f", 0, None), INVAL, 'map index out of bounds', ()),
    ("lru_lookup_batch", (99, "k", 2, "v", "f", 0), INVAL, 'map index out of bounds', ()),
    ("lru_delete_batch_device", (99, "k", 2, "f", None), INVAL, 'map index out of bounds', ()),
    ("lru_delete_batch", (99, "k", 2, "f"), INVAL, 'map index out of bounds', ()),
    ("lru_order_device", (99, None, 0, "k", "v", 2, "n", None), INVAL, 'map index out of bounds', ()),
    ("lru_order", (99, None, 0, "k", "v", 2, "n"), INVAL, 'map index out of bounds', ()),
    ("lru_evict_device", (99, None, 1, "k", "v", 2, "n", None), INVAL, 'map index out of bounds', ()),
    ("lru_evict", (99, None, 1, "k", "v", 2, "n"), INVAL, 'map index out of bounds', ()),
    # ---- wrong kind, both directions
    ("map_lookup_batch_device", ("L", "k", 2, "v", "f", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_lookup_batch_device", ("Q", "k", 2, "v", "f", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_lookup_batch", ("L", "k", 2, "v", "f"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_update_batch_device", ("L", "k", "v", 2, None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_update_batch_staged", ("L", "k", "v", 2), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_delete_batch_device", ("L", "k", 2, "f", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_delete_batch", ("L", "k", 2, "f"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_modify_batch_device", ("L", "k", 2, ADD1, 1, "v", "f", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_modify_batch", ("L", "k", 2, ADD1, 1, "v", "f"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_scan_device", ("L", None, "k", "v", 2, "n", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_scan", ("L", None, "k", "v", 2, "n"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_scan", ("Q", None, "k", "v", 2, "n"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_expire_device", ("L", None, "k", "v", 2, "n", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_expire", ("L", None, "k", "v", 2, "n"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_top_device", ("L", None, ORD, "k", "v", 2, "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_top", ("L", None, ORD, "k", "v", 2, "n", "c"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_evict_device", ("L", None, ORD, "k", "v", 2, "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_evict", ("L", None, ORD, "k", "v", 2, "n", "c"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_stats", ("L", None, ORD, "stats", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_group", ("L", None, GRP, "D", "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_group", ("H", None, GRP, "L", "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_join_device", ("L", None, JOIN, "D", "k", "v", "j", 2, "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_join_device", ("H", None, JOIN, "L", "k", "v", "j", 2, "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_join", ("L", None, JOIN, "D", "k", "v", "j", 2, "n", "c"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_join", ("H", None, JOIN, "L", "k", "v", "j", 2, "n", "c"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_compact", ("L", 0, "info", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_modify_device", ("L", None, ADD1, 1, "k", "v", 2, "n", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_modify", ("L", None, ADD1, 1, "k", "v", 2, "n"), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("lru_lookup_batch_device", ("H", "k", 2, "v", "f", 0, None), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_lookup_batch_device", ("A", "k", 2, "v", "f", 0, None), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_lookup_batch", ("H", "k", 2, "v", "f", 0), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_lookup_batch", ("A", "k", 2, "v", "f", 0), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_delete_batch_device", ("H", "k", 2, "f", None), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_delete_batch", ("H", "k", 2, "f"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_delete_batch", ("Q", "k", 2, "f"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_order_device", ("H", None, 0, "k", "v", 2, "n", None), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_order_device", ("Q", None, 0, "k", "v", 2, "n", None), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_order", ("H", None, 0, "k", "v", 2, "n"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_order", ("A", None, 0, "k", "v", 2, "n"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_evict_device", ("H", None, 1, "k", "v", 2, "n", None), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_evict", ("H", None, 1, "k", "v", 2, "n"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    # ---- ARRAY delete, expire and evict
    ("map_delete_batch_device", ("A", "k", 2, "f", None), INVAL, 'delete not available on this map type', (1,)),
    ("map_delete_batch", ("A", "k", 2, "f"), INVAL, 'delete not available on this map type', (1,)),
    ("map_expire_device", ("A", None, "k", "v", 2, "n", None), INVAL, 'delete not available on this map type', (1,)),
    ("map_expire", ("A", None, "k", "v", 2, "n"), INVAL, 'delete not available on this map type', (1,)),
    ("map_evict_device", ("A", None, ORD, "k", "v", 2, "n", "c", None), INVAL, 'delete not available on this map type', (1,)),
    ("map_evict", ("A", None, ORD, "k", "v", 2, "n", "c"), INVAL, 'delete not available on this map type', (1,)),
    ("map_join_device", ("A", None, J(0, 0, 4, 0, 1, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'delete not available on this map type', (0, 0)),
    ("map_join", ("A", None, J(0, 0, 4, 0, 1, 0), "D", "k", "v", "j", 2, "n", "c"), INVAL, 'delete not available on this map type', (0, 0)),
    # ---- null required pointer
    ("map_lookup_batch_device", ("H", None, 2, "v", "f", None), INVAL, 'null keys / values', (0,)),
    ("map_lookup_batch_device", ("H", "k", 2, None, "f", None), INVAL, 'null keys / values', (0,)),
    ("map_lookup_batch", ("H", None, 2, "v", "f"), INVAL, 'null keys / values', (0,)),
    ("map_lookup_batch", ("H", "k", 2, None, "f"), INVAL, 'null keys / values', (0,)),
    ("map_update_batch_device", ("H", None, "v", 2, None), INVAL, 'null keys / values', (0,)),
    ("map_update_batch_device", ("H", "k", None, 2, None), INVAL, 'null keys / values', (0,)),
    ("map_update_batch_staged", ("H", None, "v", 2), INVAL, 'null keys / values', (0,)),
    ("map_update_batch_staged", ("H", "k", None, 2), INVAL, 'null keys / values', (0,)),
    ("map_delete_batch_device", ("H", None, 2, "f", None), INVAL, 'null keys', (0,)),
    ("map_delete_batch", ("H", None, 2, "f"), INVAL, 'null keys', (0,)),
    ("map_modify_batch_device", ("H", None, 2, ADD1, 1, "v", "f", None), INVAL, 'null keys', (0,)),
    ("map_modify_batch", ("H", None, 2, ADD1, 1, "v", "f"), INVAL, 'null keys', (0,)),
    ("map_stats", ("H", None, ORD, None, None), INVAL, 'null stats', (1,)),
    ("map_compact", ("H", 0, None, None), INVAL, 'null compact info', (1,)),
    ("lru_lookup_batch_device", ("L", None, 2, "v", "f", 0, None), INVAL, 'null keys / values', (0,)),
    ("lru_lookup_batch_device", ("L", "k", 2, None, "f", 0, None), INVAL, 'null keys / values', (0,)),
    ("lru_lookup_batch", ("L", None, 2, "v", "f", 0), INVAL, 'null keys / values', (0,)),
    ("lru_lookup_batch", ("L", "k", 2, None, "f", 0), INVAL, 'null keys / values', (0,)),
    ("lru_delete_batch_device", ("L", None, 2, "f", None), INVAL, 'null keys', (0,)),
    ("lru_delete_batch", ("L", None, 2, "f"), INVAL, 'null keys', (0,)),
    # ---- null matched
    ("map_scan_device", ("H", None, "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("map_scan", ("H", None, "k", "v", 2, None), INVAL, 'null matched', (1,)),
    ("map_expire_device", ("H", None, "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("map_expire", ("H", None, "k", "v", 2, None), INVAL, 'null matched', (1,)),
    ("map_top_device", ("H", None, ORD, "k", "v", 2, None, "c", None), INVAL, 'null matched', (1,)),
    ("map_top", ("H", None, ORD, "k", "v", 2, None, "c"), INVAL, 'null matched', (1,)),
    ("map_evict_device", ("H", None, ORD, "k", "v", 2, None, "c", None), INVAL, 'null matched', (1,)),
    ("map_evict", ("H", None, ORD, "k", "v", 2, None, "c"), INVAL, 'null matched', (1,)),
    ("map_group", ("H", None, GRP, "D", None, "c", None), INVAL, 'null matched', (0, 0)),
    ("map_join_device", ("H", None, JOIN, "D", "k", "v", "j", 2, None, "c", None), INVAL, 'null matched', (0, 0)),
    ("map_join", ("H", None, JOIN, "D", "k", "v", "j", 2, None, "c"), INVAL, 'null matched', (0, 0)),
    ("map_modify_device", ("H", None, ADD1, 1, "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("map_modify", ("H", None, ADD1, 1, "k", "v", 2, None), INVAL, 'null matched', (1,)),
    ("lru_order_device", ("L", None, 0, "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("lru_order", ("L", None, 0, "k", "v", 2, None), INVAL, 'null matched', (1,)),
    ("lru_evict_device", ("L", None, 1, "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("lru_evict", ("L", None, 1, "k", "v", 2, None), INVAL, 'null matched', (1,)),
    # ---- count above 2^31
    ("map_lookup_batch_device", ("H", "k", BIG, "v", "f", None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_lookup_batch", ("H", "k", BIG, "v", "f"), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_update_batch_device", ("H", "k", "v", BIG, None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_update_batch_staged", ("H", "k", "v", BIG), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_delete_batch_device", ("H", "k", BIG, "f", None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_delete_batch", ("H", "k", BIG, "f"), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_modify_batch_device", ("H", "k", BIG, ADD1, 1, "v", "f", None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("map_modify_batch", ("H", "k", BIG, ADD1, 1, "v", "f"), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("lru_lookup_batch_device", ("L", "k", BIG, "v", "f", 0, None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("lru_lookup_batch", ("L", "k", BIG, "v", "f", 0), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("lru_delete_batch_device", ("L", "k", BIG, "f", None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("lru_delete_batch", ("L", "k", BIG, "f"), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    # ---- unknown flag
    ("map_compact", ("H", 2, "info", None), INVAL, 'map compact: unknown flag', (1,)),
    ("lru_lookup_batch_device", ("L", "k", 2, "v", "f", 2, None), INVAL, 'lru lookup: unknown flag', (1,)),
    ("lru_lookup_batch", ("L", "k", 2, "v", "f", 2), INVAL, 'lru lookup: unknown flag', (1,)),
    ("lru_order_device", ("L", None, 0x80000001, "k", "v", 2, "n", None), INVAL, 'lru order: unknown flag', (1,)),
    ("lru_order", ("L", None, 0x80000001, "k", "v", 2, "n"), INVAL, 'lru order: unknown flag', (1,)),
    ("lru_evict_device", ("L", None, 0x80000001, "k", "v", 2, "n", None), INVAL, 'lru order: unknown flag', (1,)),
    ("lru_evict", ("L", None, 0x80000001, "k", "v", 2, "n"), INVAL, 'lru order: unknown flag', (1,)),
    # ---- bad filter
    ("map_scan_device", ("H", F(9, 0, 8, 0, 0), "k", "v", 2, "n", None), INVAL, 'map filter: unknown op', (1,)),
    ("map_scan_device", ("H", F(1, 0, 8, 1, 0), "k", "v", 2, "n", None), INVAL, 'map filter: pad must be 0', (1,)),
    ("map_scan_device", ("H", F(1, 0, 3, 0, 0), "k", "v", 2, "n", None), INVAL, 'map filter: width must be 1, 2, 4 or 8', (1,)),
    ("map_scan_device", ("H", F(1, 1, 8, 0, 0), "k", "v", 2, "n", None), INVAL, 'map filter: the field lies outside the value', (1,)),
    ("map_scan", ("H", F(9, 0, 8, 0, 0), "k", "v", 2, "n"), INVAL, 'map filter: unknown op', (1,)),
    ("map_expire_device", ("H", F(1, 0, 8, 1, 0), "k", "v", 2, "n", None), INVAL, 'map filter: pad must be 0', (1,)),
    ("map_expire", ("H", F(1, 0, 3, 0, 0), "k", "v", 2, "n"), INVAL, 'map filter: width must be 1, 2, 4 or 8', (1,)),
    ("map_top_device", ("H", F(1, 1, 8, 0, 0), ORD, "k", "v", 2, "n", "c", None), INVAL, 'map filter: the field lies outside the value', (1,)),
    ("map_top", ("H", F(9, 0, 8, 0, 0), ORD, "k", "v", 2, "n", "c"), INVAL, 'map filter: unknown op', (1,)),
    ("map_evict_device", ("H", F(1, 0, 8, 1, 0), ORD, "k", "v", 2, "n", "c", None), INVAL, 'map filter: pad must be 0', (1,)),
    ("map_evict", ("H", F(1, 0, 3, 0, 0), ORD, "k", "v", 2, "n", "c"), INVAL, 'map filter: width must be 1, 2, 4 or 8', (1,)),
    ("map_stats", ("H", F(1, 1, 8, 0, 0), ORD, "stats", None), INVAL, 'map filter: the field lies outside the value', (1,)),
    ("map_group", ("H", F(9, 0, 8, 0, 0), GRP, "D", "n", "c", None), INVAL, 'map filter: unknown op', (1, 0)),
    ("map_join_device", ("H", F(1, 0, 8, 1, 0), JOIN, "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map filter: pad must be 0', (1, 0)),
    ("map_join", ("H", F(1, 0, 3, 0, 0), JOIN, "D", "k", "v", "j", 2, "n", "c"), INVAL, 'map filter: width must be 1, 2, 4 or 8', (1, 0)),
    ("map_modify_device", ("H", F(1, 1, 8, 0, 0), ADD1, 1, "k", "v", 2, "n", None), INVAL, 'map filter: the field lies outside the value', (1,)),
    ("map_modify", ("H", F(9, 0, 8, 0, 0), ADD1, 1, "k", "v", 2, "n"), INVAL, 'map filter: unknown op', (1,)),
    ("lru_order_device", ("L", F(1, 0, 8, 1, 0), 0, "k", "v", 2, "n", None), INVAL, 'map filter: pad must be 0', (1,)),
    ("lru_order", ("L", F(1, 0, 3, 0, 0), 0, "k", "v", 2, "n"), INVAL, 'map filter: width must be 1, 2, 4 or 8', (1,)),
    ("lru_evict_device", ("L", F(1, 1, 8, 0, 0), 1, "k", "v", 2, "n", None), INVAL, 'map filter: the field lies outside the value', (1,)),
    ("lru_evict", ("L", F(9, 0, 8, 0, 0), 1, "k", "v", 2, "n"), INVAL, 'map filter: unknown op', (1,)),
    # ---- bad order
    ("map_top_device", ("H", None, None, "k", "v", 2, "n", "c", None), INVAL, 'null map order', (1,)),
    ("map_top_device", ("H", None, O(0, 3, 0, 0), "k", "v", 2, "n", "c", None), INVAL, 'map order: width must be 1, 2, 4 or 8', (1,)),
    ("map_top_device", ("H", None, O(4, 8, 0, 0), "k", "v", 2, "n", "c", None), INVAL, 'map order: the field lies outside the value', (1,)),
    ("map_top_device", ("H", None, O(0, 8, 0, 1), "k", "v", 2, "n", "c", None), INVAL, 'map order: pad must be 0', (1,)),
    ("map_top_device", ("H", None, O(0, 8, 2, 0), "k", "v", 2, "n", "c", None), INVAL, 'map order: descending must be 0 or 1', (1,)),
    ("map_top", ("H", None, None, "k", "v", 2, "n", "c"), INVAL, 'null map order', (1,)),
    ("map_top", ("H", None, O(4, 8, 0, 0), "k", "v", 2, "n", "c"), INVAL, 'map order: the field lies outside the value', (1,)),
    ("map_evict_device", ("H", None, O(0, 3, 0, 0), "k", "v", 2, "n", "c", None), INVAL, 'map order: width must be 1, 2, 4 or 8', (1,)),
    ("map_evict_device", ("H", None, O(0, 8, 0, 1), "k", "v", 2, "n", "c", None), INVAL, 'map order: pad must be 0', (1,)),
    ("map_evict", ("H", None, O(4, 8, 0, 0), "k", "v", 2, "n", "c"), INVAL, 'map order: the field lies outside the value', (1,)),
    ("map_evict", ("H", None, O(0, 8, 2, 0), "k", "v", 2, "n", "c"), INVAL, 'map order: descending must be 0 or 1', (1,)),
    ("map_stats", ("H", None, O(0, 8, 0, 1), "stats", None), INVAL, 'map order: pad must be 0', (1,)),
    ("map_stats", ("H", None, None, "stats", None), INVAL, 'null map order', (1,)),
    # ---- bad edit
    ("map_modify_device", ("H", None, None, 1, "k", "v", 2, "n", None), INVAL, 'null map edits', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, None, 1, "v", "f", None), INVAL, 'null map edits', (1,)),
    ("map_modify_device", ("H", None, ADD1, 0, "k", "v", 2, "n", None), INVAL, 'map edit: between 1 and XE_MM_MAX_EDITS edits', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, ADD1, 0, "v", "f", None), INVAL, 'map edit: between 1 and XE_MM_MAX_EDITS edits', (1,)),
    ("map_modify_device", ("H", None, ADD1, 9, "k", "v", 2, "n", None), INVAL, 'map edit: between 1 and XE_MM_MAX_EDITS edits', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, ADD1, 9, "v", "f", None), INVAL, 'map edit: between 1 and XE_MM_MAX_EDITS edits', (1,)),
    ("map_modify_device", ("H", None, E(ED(99, 0, 8, 0, 1)), 1, "k", "v", 2, "n", None), INVAL, 'map edit: unknown op', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, E(ED(99, 0, 8, 0, 1)), 1, "v", "f", None), INVAL, 'map edit: unknown op', (1,)),
    ("map_modify_device", ("H", None, E(ED(1, 0, 8, 2, 1)), 1, "k", "v", 2, "n", None), INVAL, 'map edit: unknown flag', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, E(ED(1, 0, 8, 2, 1)), 1, "v", "f", None), INVAL, 'map edit: unknown flag', (1,)),
    ("map_modify_device", ("H", None, E(ED(1, 0, 3, 0, 1)), 1, "k", "v", 2, "n", None), INVAL, 'map edit: width must be 1, 2, 4 or 8', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, E(ED(1, 0, 3, 0, 1)), 1, "v", "f", None), INVAL, 'map edit: width must be 1, 2, 4 or 8', (1,)),
    ("map_modify_device", ("H", None, E(ED(1, 4, 8, 0, 1)), 1, "k", "v", 2, "n", None), INVAL, 'map edit: the field lies outside the value', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, E(ED(1, 4, 8, 0, 1)), 1, "v", "f", None), INVAL, 'map edit: the field lies outside the value', (1,)),
    ("map_modify_device", ("H", None, E(ED(1, 0, 4, 1, 6)), 1, "k", "v", 2, "n", None), INVAL, 'map edit: the operand field lies outside the value', (1,)),
    ("map_modify_batch_device", ("H", "k", 2, E(ED(1, 0, 4, 1, 6)), 1, "v", "f", None), INVAL, 'map edit: the operand field lies outside the value', (1,)),
    ("map_modify", ("H", None, None, 1, "k", "v", 2, "n"), INVAL, 'null map edits', (1,)),
    ("map_modify", ("H", None, E(ED(99, 0, 8, 0, 1)), 1, "k", "v", 2, "n"), INVAL, 'map edit: unknown op', (1,)),
    ("map_modify_batch", ("H", "k", 2, ADD1, 0, "v", "f"), INVAL, 'map edit: between 1 and XE_MM_MAX_EDITS edits', (1,)),
    ("map_modify_batch", ("H", "k", 2, E(ED(1, 0, 8, 2, 1)), 1, "v", "f"), INVAL, 'map edit: unknown flag', (1,)),
    # ---- bad group spec
    ("map_group", ("H", None, None, "D", "n", "c", None), INVAL, 'null map group spec', (0, 0)),
    ("map_group", ("H", None, G(2, 0, 4, 0, 8, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: from must be XE_MG_KEY or XE_MG_VALUE', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 8, 0, 8, 1), "D", "n", "c", None), INVAL, 'map group: pad must be 0', (0, 0)),
    ("map_group", ("H", None, G(0, 2, 4, 0, 8, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: the group bytes lie outside the source key / value', (0, 0)),
    ("map_group", ("H", None, G(1, 6, 4, 0, 8, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: the group bytes lie outside the source key / value', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 0, 0, 8, 0, NONE, 0), "Z", "n", "c", None), INVAL, 'map group: the destination has no key bytes', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 2, 0, 8, 0, 8, 0), "D", "n", "c", None), INVAL, "map group: len must be the destination's key_size", (0, 0)),
    ("map_group", ("H", None, G(0, 0, 3, 0, 8, 0, 8, 0), "B", "n", "c", None), INVAL, 'map group: len must be 1, 2 or 4 for an ARRAY destination', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 8, NONE, NONE, 0), "D", "n", "c", None), INVAL, 'map group: no accumulator', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 0, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: a sum needs a measure', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 3, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: measure width must be 1, 2, 4 or 8', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 4, 8, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: the measure lies outside the source value', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 8, 0, NONE, 0), "E", "n", "c", None), INVAL, "map group: the destination's value_size must be a multiple of 8", (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 8, 4, 8, 0), "D", "n", "c", None), INVAL, 'map group: an accumulator must be 8-byte aligned inside the destination value', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 8, 0, 16, 0), "D", "n", "c", None), INVAL, 'map group: an accumulator must be 8-byte aligned inside the destination value', (0, 0)),
    ("map_group", ("H", None, G(0, 0, 4, 0, 8, 8, 8, 0), "D", "n", "c", None), INVAL, 'map group: the accumulators overlap', (0, 0)),
    ("map_group", ("H", None, GRP, "H", "n", "c", None), INVAL, 'map group: source and destination are one map', (0, 0)),
    # ---- bad join spec
    ("map_join_device", ("H", None, None, "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'null map join spec', (0, 0)),
    ("map_join_device", ("H", None, J(2, 0, 4, 0, 0, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: from must be XE_MG_KEY or XE_MG_VALUE', (0, 0)),
    ("map_join_device", ("H", None, J(0, 0, 4, 2, 0, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: mode must be XE_MJ_PRESENT or XE_MJ_ABSENT', (0, 0)),
    ("map_join_device", ("H", None, J(0, 0, 4, 0, 2, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: unknown flag', (0, 0)),
    ("map_join_device", ("H", None, J(0, 0, 4, 0, 0, 1), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: pad must be 0', (0, 0)),
    ("map_join_device", ("H", None, J(0, 2, 4, 0, 0, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: the join bytes lie outside the source key / value', (0, 0)),
    ("map_join_device", ("H", None, J(1, 6, 4, 0, 0, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: the join bytes lie outside the source key / value', (0, 0)),
    ("map_join_device", ("H", None, J(0, 0, 0, 0, 0, 0), "Z", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: the other map has no key bytes', (0, 0)),
    ("map_join_device", ("H", None, J(0, 0, 2, 0, 0, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, "map join: len must be the other map's key_size", (0, 0)),
    ("map_join_device", ("H", None, J(0, 0, 3, 0, 0, 0), "B", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: len must be 1, 2 or 4 for an ARRAY other map', (0, 0)),
    ("map_join", ("H", None, None, "D", "k", "v", "j", 2, "n", "c"), INVAL, 'null map join spec', (0, 0)),
    ("map_join", ("H", None, J(0, 0, 4, 0, 2, 0), "D", "k", "v", "j", 2, "n", "c"), INVAL, 'map join: unknown flag', (0, 0)),
    # ---- write during an open epoch
    ("map_update_batch_device", ("epoch", "H", "k", "v", 2, None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_update_batch_staged", ("epoch", "H", "k", "v", 2), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_delete_batch_device", ("epoch", "H", "k", 2, "f", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_delete_batch", ("epoch", "H", "k", 2, "f"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_modify_batch_device", ("epoch", "H", "k", 2, ADD1, 1, "v", "f", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_modify_batch", ("epoch", "H", "k", 2, ADD1, 1, "v", "f"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_expire_device", ("epoch", "H", None, "k", "v", 2, "n", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_expire", ("epoch", "H", None, "k", "v", 2, "n"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_evict_device", ("epoch", "H", None, ORD, "k", "v", 2, "n", "c", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_evict", ("epoch", "H", None, ORD, "k", "v", 2, "n", "c"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_group", ("epoch", "H", None, GRP, "D", "n", "c", None), INVAL, 'map writes are refused while a shard epoch is open', (0, 0)),
    ("map_compact", ("epoch", "H", 0, "info", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_modify_device", ("epoch", "H", None, ADD1, 1, "k", "v", 2, "n", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_modify", ("epoch", "H", None, ADD1, 1, "k", "v", 2, "n"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_lookup_batch_device", ("epoch", "L", "k", 2, "v", "f", 0, None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_lookup_batch", ("epoch", "L", "k", 2, "v", "f", 0), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_delete_batch_device", ("epoch", "L", "k", 2, "f", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_delete_batch", ("epoch", "L", "k", 2, "f"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_evict_device", ("epoch", "L", None, 1, "k", "v", 2, "n", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_evict", ("epoch", "L", None, 1, "k", "v", 2, "n"), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_join_device", ("epoch", "H", None, J(0, 0, 4, 0, 1, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map writes are refused while a shard epoch is open', (0, 0)),
    ("map_join", ("epoch", "H", None, J(0, 0, 4, 0, 1, 0), "D", "k", "v", "j", 2, "n", "c"), INVAL, 'map writes are refused while a shard epoch is open', (0, 0)),
    # ---- read during an open epoch
    ("map_lookup_batch_device", ("epoch", "H", "k", 2, "v", "f", None), OK, None, (0,)),
    ("map_scan", ("epoch", "H", None, "k", "v", 2, "n"), OK, None, (0,)),
    ("map_stats", ("epoch", "H", None, ORD, "stats", None), OK, None, (0,)),
    ("lru_order_device", ("epoch", "L", None, 0, "k", "v", 2, "n", None), OK, None, (0,)),
    ("lru_lookup_batch_device", ("epoch", "L", "k", 2, "v", "f", 1, None), OK, None, (0,)),
    ("lru_lookup_batch", ("epoch", "L", "k", 2, "v", "f", 1), OK, None, (0,)),
    ("map_compact", ("epoch", "H", 1, "info", None), OK, None, (0,)),
    # ---- count 0
    ("map_lookup_batch_device", ("H", "k", 0, "v", "f", None), OK, None, (0,)),
    ("map_lookup_batch_device", ("H", None, 0, "v", "f", None), OK, None, (0,)),
    ("map_lookup_batch", ("H", "k", 0, "v", "f"), OK, None, (0,)),
    ("map_lookup_batch", ("H", None, 0, "v", "f"), OK, None, (0,)),
    ("map_update_batch_device", ("H", "k", "v", 0, None), OK, None, (0,)),
    ("map_update_batch_device", ("H", None, "v", 0, None), OK, None, (0,)),
    ("map_update_batch_staged", ("H", "k", "v", 0), OK, None, (0,)),
    ("map_update_batch_staged", ("H", None, "v", 0), OK, None, (0,)),
    ("map_delete_batch_device", ("H", "k", 0, "f", None), OK, None, (0,)),
    ("map_delete_batch_device", ("H", None, 0, "f", None), OK, None, (0,)),
    ("map_delete_batch", ("H", "k", 0, "f"), OK, None, (0,)),
    ("map_delete_batch", ("H", None, 0, "f"), OK, None, (0,)),
    ("map_modify_batch_device", ("H", "k", 0, ADD1, 1, "v", "f", None), OK, None, (0,)),
    ("map_modify_batch_device", ("H", None, 0, ADD1, 1, "v", "f", None), OK, None, (0,)),
    ("map_modify_batch", ("H", "k", 0, ADD1, 1, "v", "f"), OK, None, (0,)),
    ("map_modify_batch", ("H", None, 0, ADD1, 1, "v", "f"), OK, None, (0,)),
    ("lru_lookup_batch_device", ("L", "k", 0, "v", "f", 0, None), OK, None, (0,)),
    ("lru_lookup_batch_device", ("L", None, 0, "v", "f", 0, None), OK, None, (0,)),
    ("lru_lookup_batch", ("L", "k", 0, "v", "f", 0), OK, None, (0,)),
    ("lru_lookup_batch", ("L", None, 0, "v", "f", 0), OK, None, (0,)),
    ("lru_delete_batch_device", ("L", "k", 0, "f", None), OK, None, (0,)),
    ("lru_delete_batch_device", ("L", None, 0, "f", None), OK, None, (0,)),
    ("lru_delete_batch", ("L", "k", 0, "f"), OK, None, (0,)),
    ("lru_delete_batch", ("L", None, 0, "f"), OK, None, (0,)),
    # ---- two refusals at once
    ("map_delete_batch_device", ("A", None, 2, "f", None), INVAL, 'delete not available on this map type', (0,)),
    ("map_delete_batch", ("A", None, 2, "f"), INVAL, 'delete not available on this map type', (0,)),
    ("map_delete_batch_device", ("A", "k", 0, "f", None), INVAL, 'delete not available on this map type', (0,)),
    ("map_delete_batch_device", ("epoch", "A", "k", 2, "f", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_lookup_batch_device", ("L", "k", BIG, "v", "f", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_lookup_batch_device", ("H", None, BIG, "v", "f", None), INVAL, 'null keys / values', (0,)),
    ("map_update_batch_device", ("epoch", "L", "k", "v", 2, None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0,)),
    ("map_update_batch_device", ("epoch", "H", "k", "v", BIG, None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_update_batch_staged", ("epoch", "H", "k", None, 2), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_modify_batch_device", ("H", None, 2, None, 1, "v", "f", None), INVAL, 'null keys', (0,)),
    ("map_modify_batch_device", ("H", "k", 0, None, 1, "v", "f", None), INVAL, 'null map edits', (0,)),
    ("map_modify_batch", ("H", "k", 0, None, 1, "v", "f"), INVAL, 'null map edits', (0,)),
    ("map_expire_device", ("A", None, "k", "v", 2, None, None), INVAL, 'delete not available on this map type', (1,)),
    ("map_expire", ("A", F(9, 0, 8, 0, 0), "k", "v", 2, "n"), INVAL, 'delete not available on this map type', (1,)),
    ("map_scan_device", ("H", F(9, 0, 8, 0, 0), "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("map_top_device", ("H", F(9, 0, 8, 0, 0), None, "k", "v", 2, "n", "c", None), INVAL, 'map filter: unknown op', (1,)),
    ("map_top", ("H", None, None, "k", "v", 2, None, "c"), INVAL, 'null matched', (1,)),
    ("map_evict_device", ("A", None, None, "k", "v", 2, "n", "c", None), INVAL, 'delete not available on this map type', (1,)),
    ("map_stats", ("H", None, None, None, None), INVAL, 'null stats', (1,)),
    ("map_group", ("H", None, None, "D", None, "c", None), INVAL, 'null map group spec', (0, 0)),
    ("map_group", ("H", None, None, "L", "n", "c", None), UNSUPPORTED, 'batched device map operations serve ARRAY and HASH maps only', (0, 0)),
    ("map_group", ("H", F(9, 0, 8, 0, 0), G(2, 0, 4, 0, 8, 0, 8, 0), "D", "n", "c", None), INVAL, 'map group: from must be XE_MG_KEY or XE_MG_VALUE', (0, 0)),
    ("map_group", ("epoch", "H", None, None, "D", "n", "c", None), INVAL, 'map writes are refused while a shard epoch is open', (0, 0)),
    ("map_join_device", ("H", None, None, "D", "k", "v", "j", 2, None, "c", None), INVAL, 'null map join spec', (0, 0)),
    ("map_join_device", ("H", F(9, 0, 8, 0, 0), J(2, 0, 4, 0, 0, 0), "D", "k", "v", "j", 2, "n", "c", None), INVAL, 'map join: from must be XE_MG_KEY or XE_MG_VALUE', (0, 0)),
    ("map_join", ("epoch", "A", None, J(0, 0, 4, 0, 1, 0), "D", "k", "v", "j", 2, "n", "c"), INVAL, 'map writes are refused while a shard epoch is open', (0, 0)),
    ("map_compact", ("H", 2, None, None), INVAL, 'null compact info', (1,)),
    ("map_compact", ("epoch", "A", 0, "info", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("map_modify_device", ("H", None, None, 1, "k", "v", 2, None, None), INVAL, 'null matched', (1,)),
    ("map_modify_device", ("H", F(9, 0, 8, 0, 0), None, 1, "k", "v", 2, "n", None), INVAL, 'map filter: unknown op', (1,)),
    ("map_modify", ("epoch", "H", None, ADD1, 1, "k", "v", 2, None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_lookup_batch_device", ("L", None, 2, "v", "f", 2, None), INVAL, 'lru lookup: unknown flag', (0,)),
    ("lru_lookup_batch_device", ("L", "k", 0, "v", "f", 2, None), INVAL, 'lru lookup: unknown flag', (0,)),
    ("lru_lookup_batch_device", ("L", "k", BIG, "v", "f", 2, None), INVAL, 'batched map operation: more than 2^31 keys', (0,)),
    ("lru_lookup_batch_device", ("epoch", "L", "k", 2, "v", "f", 2, None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_lookup_batch", ("H", "k", 2, "v", "f", 3), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_lookup_batch", ("L", None, 2, "v", "f", 2), INVAL, 'lru lookup: unknown flag', (0,)),
    ("lru_lookup_batch", ("epoch", "L", "k", BIG, "v", "f", 0), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_delete_batch_device", ("epoch", "L", None, 2, "f", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_delete_batch", ("epoch", "H", "k", 2, "f"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
    ("lru_order_device", ("L", None, 2, "k", "v", 2, None, None), INVAL, 'lru order: unknown flag', (1,)),
    ("lru_order", ("L", F(9, 0, 8, 0, 0), 0, "k", "v", 2, None), INVAL, 'null matched', (1,)),
    ("lru_evict_device", ("epoch", "L", None, 2, "k", "v", 2, "n", None), INVAL, 'map writes are refused while a shard epoch is open', (0,)),
    ("lru_evict", ("epoch", "H", None, 1, "k", "v", 2, "n"), INVAL, 'the xe_lru_ calls serve LRU_HASH maps only', (0,)),
)


def ident(row):
    call, args = row[0], row[1]
    return call + "-" + "-".join("null" if a is None else a if isinstance(a, str) else str(a) if isinstance(a, int) else type(a).__name__
                                 for a in args)


def check(lib, row, device_buffer=None):
    call, args, rc, text, uploads = row
    assert run_row(lib, call, args, device_buffer) == (rc, text, uploads)


@pytest.mark.parametrize("row", ROWS, ids=[f"{i:03d}-{ident(r)}" for i, r in enumerate(ROWS)])
def test_refusal(hostsim_lib, row):
    check(hostsim_lib, row)


@pytest.mark.gpu
def test_refusals_on_the_product_library(gpu_lib):
    import torch

    def device_buffer(nbytes):
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the call on the VM's)
        return t, t.data_ptr()

    for row in ROWS:
        check(gpu_lib, row, device_buffer)
