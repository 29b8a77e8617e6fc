"""Host-side mirror of gobpfld's `emulator` package API over the MI355X device emulator.

    vm = VM(Settings())                      # emulator.NewVM            (emulator/vm.go:30-48)
    prog = vm.add_raw_program(insns)         # VM.AddRawProgram          (emulator/vm.go:61-73)
    m = vm.add_map(MapDef(...), initial)     # VM.AddMap/AddAbstractMap  (emulator/vm.go:75-98)
    vm.set_entrypoint(prog)                  # VM.SetEntrypoint          (emulator/vm.go:100-108)
    res = vm.run_batch(umem, descs)          # Reset + R1=ctx + Run per packet (vm.go:110-246)
    vm.map_dump(m)                           # final map state (Map.Keys + Lookup)

Errors raise EmulatorError carrying the library's message (the Go API returns `error`).
Per-packet failures never raise: they are reported in the result's `status`.
The product library is the HIP one; passing another `lib` is for tests only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N

STATUS = {0: "OK", 1: "VMERR", 2: "PANIC", 3: "BUDGET", 4: "UNSUPPORTED"}
MAP_HASH, MAP_ARRAY, MAP_PROG_ARRAY, MAP_PERF_EVENT_ARRAY, MAP_PERCPU_HASH, MAP_PERCPU_ARRAY = 1, 2, 3, 4, 5, 6
MAP_LRU_HASH, MAP_LRU_PERCPU_HASH, MAP_ARRAY_OF_MAPS, MAP_HASH_OF_MAPS, MAP_QUEUE, MAP_STACK = 9, 10, 12, 13, 22, 23
ARRAY_TYPES = (MAP_ARRAY, MAP_PERCPU_ARRAY, MAP_PROG_ARRAY, MAP_ARRAY_OF_MAPS)
HASH_TYPES = (MAP_HASH, MAP_PERCPU_HASH, MAP_HASH_OF_MAPS, MAP_LRU_HASH, MAP_LRU_PERCPU_HASH)
LIST_TYPES = (MAP_QUEUE, MAP_STACK, MAP_PERF_EVENT_ARRAY)
MODE_AUTO, MODE_PARALLEL, MODE_SEQUENTIAL, MODE_KEYED = 0, 1, 2, 3  # MODE_KEYED: mode_used only
MODE_CANCELLED = 4  # mode_used of a pipelined batch VM.cancel dropped
MODE_SEGMENTS = 5  # mode_used: packet-order segments, each in parallel (a list position after an earlier push)
E_HOST_HELPER, E_IN_HELPER = 17, 0x80
ENGINE_AUTO, ENGINE_INTERP, ENGINE_JIT = 0, 1, 2


class EmulatorError(RuntimeError):
    def __init__(self, rc: int, msg: str):
        super().__init__(f"{msg} (rc={rc})")
        self.rc = rc


@dataclass
class MapDef:
    type: int
    key_size: int
    value_size: int
    max_entries: int
    flags: int = 0


MF_ALL, MF_EQ, MF_NE, MF_LT, MF_LE, MF_GT, MF_GE, MF_ANYBITS, MF_NOBITS = range(9)  # XE_MF_* (include/xdpemu.h)


@dataclass
class MapFilter:
    """xe_map_filter: `op` applied to the unsigned little-endian field of `width` bytes at byte `offset`
    of the value, against `operand` (VM.map_scan / VM.map_expire)."""
    op: int = MF_ALL
    offset: int = 0
    width: int = 8
    operand: int = 0


@dataclass
class MapOrder:
    """xe_map_order: rank by the unsigned little-endian field of `width` bytes at byte `offset` of the
    value, largest first when `descending` (VM.map_top / VM.map_evict; the field of VM.map_stats)."""
    offset: int = 0
    width: int = 8
    descending: bool = True


MM_SET, MM_ADD, MM_SUB, MM_ADD_SAT, MM_SUB_SAT, MM_AND, MM_OR, MM_XOR, MM_MIN, MM_MAX, MM_SHR = range(11)  # XE_MM_*
MM_OPERAND_FIELD = 1  # XE_MM_OPERAND_FIELD
MM_MAX_EDITS = 8  # XE_MM_MAX_EDITS


@dataclass
class MapEdit:
    """xe_map_edit: `op` applied to the unsigned little-endian field of `width` bytes at byte `offset` of the
    value, with `operand`, or, when `operand_field`, with the field of the same width at byte `operand` of the
    same value (VM.map_modify / VM.map_modify_batch)."""
    op: int = MM_SET
    offset: int = 0
    width: int = 8
    operand: int = 0
    operand_field: bool = False


MG_KEY, MG_VALUE, MG_NONE = 0, 1, 0xffffffff  # XE_MG_* (include/xdpemu.h)
MC_COUNT_ONLY = 1  # XE_MC_COUNT_ONLY
LRU_PEEK = 1  # XE_LRU_PEEK (VM.lru_lookup_batch)
LRU_OLDEST_FIRST = 1  # XE_LRU_OLDEST_FIRST (VM.lru_order / VM.lru_evict)


@dataclass
class MapGroup:
    """xe_map_group_spec: group by the `len` bytes at byte `offset` of the source entry's key (`from_` MG_KEY;
    an ARRAY source's index as a u32) or value (MG_VALUE); the destination's u64 at `count_off` gains the
    group's entries, the one at `sum_off` the sum of their measures, `measure_width` bytes at `measure_off` of
    the source value (VM.map_group). MG_NONE: no such accumulator."""
    from_: int = MG_KEY
    offset: int = 0
    len: int = 4
    count_off: int = 0
    sum_off: int = MG_NONE
    measure_off: int = 0
    measure_width: int = 0


MJ_PRESENT, MJ_ABSENT = 0, 1  # XE_MJ_* modes (include/xdpemu.h)
MJ_REMOVE = 1  # XE_MJ_REMOVE


@dataclass
class MapJoin:
    """xe_map_join_spec: the join key is the `len` bytes at byte `offset` of the source entry's key (`from_` MG_KEY;
    an ARRAY source's index as a u32) or value (MG_VALUE); `mode` MJ_PRESENT keeps the entries whose join key is an
    entry of the other map, MJ_ABSENT those whose key is not (VM.map_join)."""
    from_: int = MG_KEY
    offset: int = 0
    len: int = 4
    mode: int = MJ_PRESENT


@dataclass
class Settings:
    max_steps: int = 1 << 20
    ingress_ifindex: int = 1
    rx_queue_index: int = 0
    device: int = 0
    mode: int = MODE_AUTO
    engine: int = 0  # ENGINE_AUTO


@dataclass
class BatchResult:
    results: np.ndarray        # structured (status, r0_kind, code, pc, r0)
    verdicts: np.ndarray       # uint32(R0)
    regs: np.ndarray | None    # structured parity records or None
    stats: dict


def initial_image(d: MapDef, data: dict) -> bytes | None:
    """AbstractMap.InitialData ({int key: bytes value}, map_abstract.go:33) as the flat image xe_add_map
    takes, copied the way ArrayMap.Init does (emulator/maps_array.go:19-44): value k lands at
    k*ValueSize and runs on into later entries when longer (keys applied in ascending order; Go's map
    order is random and only matters for overlapping copies). Only ARRAY / PERCPU_ARRAY receive
    InitialData (AbstractMapToVM, emulator/maps.go:101-108); other types get None."""
    if data is None or d.type not in (MAP_ARRAY, MAP_PERCPU_ARRAY):
        return None
    size = d.value_size * d.max_entries
    img = bytearray(size)
    for k in sorted(data):
        if not isinstance(k, int):
            raise TypeError("the key type of the initial data must be an int")
        v = bytes(data[k])
        off = k * d.value_size
        if k < 0 or off > size:
            raise ValueError(f"initial data key {k} outside the map")
        img[off:off + len(v)] = v[: size - off]
    return bytes(img)


def _wrap64(v: int) -> int:
    """a Python int as the int64 R0 a helper returns (two's complement wrap)"""
    v = int(v) & ((1 << 64) - 1)
    return v - (1 << 64) if v >> 63 else v


def _stats_dict(s: N.BatchStats) -> dict:
    return {"packets": s.packets, "steps": s.steps, "status_count": list(s.status_count),
            "mode_used": s.mode_used, "conflict": s.conflict, "kernel_ms": s.kernel_ms,
            "total_ms": s.total_ms, "engine_used": s.engine_used, "grid_blocks": s.grid_blocks}


class PendingBatch:
    """A batch queued by VM.run_batch_device_async; owns the statistics record the library fills."""

    def __init__(self, vm: "VM", st: N.BatchStats):
        self.vm, self._st = vm, st

    def stats(self) -> dict:
        self.vm.sync()
        return _stats_dict(self._st)


class VM:
    def __init__(self, settings: Settings | None = None, lib: N.Lib | None = None):
        self.lib = lib or N.product()
        s = settings or Settings()
        cs = N.Settings()
        self.lib.default_settings(C.byref(cs)) if self.lib.has("default_settings") else None
        cs.stack_frame_size, cs.max_stack_frames = 256, 8
        cs.max_steps, cs.ingress_ifindex, cs.rx_queue_index = s.max_steps, s.ingress_ifindex, s.rx_queue_index
        cs.device, cs.mode, cs.engine = s.device, s.mode, s.engine
        self.settings = s
        h = C.c_void_p()
        rc = self.lib.create(C.byref(cs), C.byref(h))
        if rc:
            raise EmulatorError(rc, "create VM")
        self.h = h
        self.map_defs: dict[int, MapDef] = {}
        self._pending: list = []  # pipelined batches whose statistics the library still writes
        self._helpers: dict[int, object] = {}  # ctypes callbacks of the host helpers (kept alive)

    def close(self) -> None:
        if self.h:
            self.lib.destroy(self.h)
            self.h = None
            self._pending.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            raise EmulatorError(rc, f"{what}: {self.lib.last_error(self.h).decode(errors='replace')}")

    # ---- programs / maps
    def add_raw_program(self, insns) -> int:
        arr = np.ascontiguousarray(np.asarray(insns, dtype=np.uint64))
        idx = C.c_int32()
        self._check(self.lib.add_raw_program(self.h, arr.ctypes.data, len(arr), C.byref(idx)), "add raw program")
        return idx.value

    def set_entrypoint(self, idx: int) -> None:
        self._check(self.lib.set_entrypoint(self.h, idx), "set entrypoint")

    def add_map(self, d: MapDef, initial: bytes | np.ndarray | dict | None = None) -> int:
        """AddAbstractMap; `initial` is a flat image or an InitialData dict (initial_image)."""
        if isinstance(initial, dict):
            initial = initial_image(d, initial)
        md = N.MapDef(d.type, d.key_size, d.value_size, d.max_entries, d.flags)
        buf = None if initial is None else np.frombuffer(bytes(initial), dtype=np.uint8)
        idx = C.c_int32()
        self._check(self.lib.add_map(self.h, C.byref(md), None if buf is None else buf.ctypes.data,
                                     0 if buf is None else len(buf), C.byref(idx)), "add map")
        self.map_defs[idx.value] = d
        return idx.value

    def map_update(self, m: int, key: bytes, value: bytes) -> None:
        d = self.map_defs[m]
        k = bytes(key).ljust(max(d.key_size, 4), b"\0")
        v = bytes(value).ljust(d.value_size, b"\0")
        self._check(self.lib.map_update(self.h, m, k, v), "map update")

    def map_update_batch(self, m: int, keys: np.ndarray, values: np.ndarray) -> None:
        """Bulk update: keys (n, key_size) and values (n, value_size) uint8 arrays."""
        d = self.map_defs[m]
        ks = d.key_size if d.type in HASH_TYPES else 4
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, ks)
        v = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, d.value_size)
        assert len(k) == len(v)
        self._check(self.lib.map_update_batch(self.h, m, k.ctypes.data, v.ctypes.data, len(k)), "map update batch")

    def map_lookup(self, m: int, key: bytes) -> bytes | None:
        d = self.map_defs[m]
        k = bytes(key).ljust(max(d.key_size, 4), b"\0")
        out = C.create_string_buffer(max(d.value_size, 1))
        rc = self.lib.map_lookup(self.h, m, k, out)
        self._check(rc, "map lookup")
        return out.raw[: d.value_size] if rc == 1 else None

    def map_delete(self, m: int, key: bytes) -> None:
        d = self.map_defs[m]
        self._check(self.lib.map_delete(self.h, m, bytes(key).ljust(max(d.key_size, 4), b"\0")), "map delete")

    def map_dump(self, m: int):
        """ARRAY -> raw bytes (ValueSize*MaxEntries); HASH / LRU_HASH -> (keys[n,ks], values[n,vs]) sorted
        by key; QUEUE / STACK / PERF_EVENT_ARRAY -> list of records (bytes) in list order."""
        d = self.map_defs[m]
        if d.type in LIST_TYPES:
            return self.map_dump_list(m)
        cnt = C.c_uint64()
        self._check(self.lib.map_dump(self.h, m, None, None, 0, C.byref(cnt)), "map dump")
        n = cnt.value
        if d.type in ARRAY_TYPES:
            raw = np.zeros(d.value_size * d.max_entries, dtype=np.uint8)
            self._check(self.lib.map_dump(self.h, m, raw.ctypes.data, None, n, C.byref(cnt)), "map dump")
            return raw.tobytes()
        keys = np.zeros((n, d.key_size), dtype=np.uint8)
        vals = np.zeros((n, d.value_size), dtype=np.uint8)
        self._check(self.lib.map_dump(self.h, m, keys.ctypes.data if n else None,
                                      vals.ctypes.data if n else None, n, C.byref(cnt)), "map dump")
        return keys, vals

    def map_dump_list(self, m: int) -> list[bytes]:
        """QUEUE / STACK / PERF_EVENT_ARRAY records in the order of the Go Values / Events slice."""
        cnt, nb = C.c_uint64(), C.c_uint64()
        self._check(self.lib.map_dump_list(self.h, m, None, 0, None, 0, C.byref(cnt), C.byref(nb)), "map dump list")
        data = np.zeros(max(1, nb.value), dtype=np.uint8)
        lens = np.zeros(max(1, cnt.value), dtype=np.uint32)
        self._check(self.lib.map_dump_list(self.h, m, data.ctypes.data, nb.value, lens.ctypes.data, cnt.value,
                                           C.byref(cnt), C.byref(nb)), "map dump list")
        out, off = [], 0
        for ln in lens[: cnt.value]:
            out.append(data[off: off + int(ln)].tobytes())
            off += int(ln)
        return out

    def map_lru_order(self, m: int) -> list[bytes]:
        """LRU_HASH UsageList keys, most recently used first (maps_hash_lru.go:21-24)."""
        d = self.map_defs[m]
        cnt = C.c_uint64()
        self._check(self.lib.map_lru_order(self.h, m, None, 0, C.byref(cnt)), "map lru order")
        keys = np.zeros((max(1, cnt.value), d.key_size), dtype=np.uint8)
        self._check(self.lib.map_lru_order(self.h, m, keys.ctypes.data, cnt.value, C.byref(cnt)), "map lru order")
        return [keys[i].tobytes() for i in range(cnt.value)]

    def map_push(self, m: int, value: bytes) -> None:
        """QueueMap/StackMap.Push of one value_size element from userspace."""
        d = self.map_defs[m]
        self._check(self.lib.map_push(self.h, m, bytes(value).ljust(d.value_size, b"\0")), "map push")

    def map_count(self, m: int) -> int:
        """xe_map_count: the map's live entries (HASH / LRU_HASH), elements (QUEUE / STACK) or events."""
        n = C.c_uint64(0)
        self._check(self.lib.map_count(self.h, m, C.byref(n)), "map count")
        return int(n.value)

    # ---- batched map access on the device copy (ARRAY / HASH; xe_map_*_batch_device). Keys and values
    # are uint8 numpy arrays, staged through the VM's device buffers, or CUDA tensors, whose device
    # addresses are passed through (the results are then tensors on the same device).
    @staticmethod
    def _is_dev(x) -> bool:
        return hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))

    def _key_size(self, m: int) -> int:
        d = self.map_defs[m]
        return 4 if d.type in ARRAY_TYPES else d.key_size  # (list maps: the library refuses them)

    def _synced_device(self, tensor=None):
        """The device of `tensor` (None: the VM's), once whatever torch has queued on its current stream there is
        complete: the calls run on the VM's stream."""
        import torch
        dev = torch.device("cuda", self.settings.device) if tensor is None else tensor.device
        torch.cuda.current_stream(dev).synchronize()
        return dev

    def _mo_keys(self, m: int, keys):
        ks = self._key_size(m)
        if self._is_dev(keys):
            import torch
            k = keys.contiguous().view(torch.uint8).reshape(-1)
            self._synced_device(k)
        else:
            k = np.ascontiguousarray(keys).view(np.uint8).reshape(-1)
        n = len(k) // ks if ks else len(keys)
        assert n * ks == len(k), "keys: a whole number of key_size-byte keys"
        return k, n

    @staticmethod
    def _c_filter(flt):
        """(the xe_map_filter of `flt`, which has to outlive the call; what to pass for it)."""
        cf = None if flt is None else N.MapFilter(flt.op, flt.offset, flt.width, 0, flt.operand)
        return cf, None if cf is None else C.byref(cf)

    @staticmethod
    def _out(shape, dev):
        """(an output array of `shape`, what to pass for it): a CUDA tensor on `dev`, or with dev None zeros on the
        host. The calls write every entry they report, so the tensor needs no fill kernel on torch's stream, which the
        VM's stream could overtake. An output of no rows is passed as NULL on either side (the keyed host forms used
        to pass the empty array's address): a call of no keys or no room returns before it looks at the pointer."""
        if dev is None:
            a = np.zeros(shape, dtype=np.uint8)
            return a, a.ctypes.data if shape[0] else None
        import torch
        a = torch.empty(shape, dtype=torch.uint8, device=dev)
        return a, a.data_ptr() or None

    def _keyed(self, m: int, keys, name: str, what: str, values: bool = True, pre=(), post=()):
        """A keyed call `name` (with _device for CUDA keys): the outputs (values[n, value_size] if `values`, found[n]).
        pre / post: the call's own arguments in front of and behind the outputs."""
        k, n = self._mo_keys(m, keys)
        dev = k.device if self._is_dev(k) else None
        outs = [self._out((n, self.map_defs[m].value_size), dev)] if values else []
        outs.append(self._out((n,), dev))
        ptrs = [p for _, p in outs]
        if dev is None:
            rc = getattr(self.lib, name)(self.h, m, k.ctypes.data, n, *pre, *ptrs, *post)
        else:
            rc = getattr(self.lib, name + "_device")(self.h, m, k.data_ptr() or None, n, *pre, *ptrs, *post, None)
        self._check(rc, what)
        return tuple(a for a, _ in outs)

    def _rows(self, what: str, n, widths, cap, on_device: bool, call, count=None, rows: int | None = None):
        """A walk call that reports rows: [output[r, width] for width in widths] + [matched], r = min(matched, cap).
        call(*pointers, cap) and count() (run first when cap is None: then every match is fetched) make the library
        call and return its code; n is the c_uint64 they have matched written to. rows: room for this many rows
        instead of cap."""
        dev = self._synced_device() if on_device else None
        if cap is None:  # count first, then fetch all
            self._check(count(), what)
            cap = n.value
        outs = [self._out((cap if rows is None else rows, w), dev) for w in widths]
        self._check(call(*[p for _, p in outs], cap), what)
        r = min(int(n.value), cap)  # (the call writes the r entries it reports; the rest is cut off)
        return [a[:r] for a, _ in outs] + [int(n.value)]

    def map_lookup_batch(self, m: int, keys):
        """(values[n, value_size], found[n]) of n keys, read from the device copy of the map."""
        return self._keyed(m, keys, "map_lookup_batch", "map lookup batch")

    def map_update_batch_device(self, m: int, keys, values) -> None:
        """All-or-nothing update of n keys on the device copy (xe_map_update_batch_device): the result of
        map_update key by key in order, or an error and an unchanged map."""
        d = self.map_defs[m]
        k, n = self._mo_keys(m, keys)
        if self._is_dev(k):
            import torch
            assert self._is_dev(values), "keys and values: both on the device, or both on the host"
            v = values.contiguous().view(torch.uint8).reshape(-1)
            assert len(v) == n * d.value_size
            self._synced_device(v)
            rc = self.lib.map_update_batch_device(self.h, m, k.data_ptr() or None, v.data_ptr() or None, n, None)
        else:
            v = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
            assert len(v) == n * d.value_size
            rc = self.lib.map_update_batch_staged(self.h, m, k.ctypes.data, v.ctypes.data, n)
        self._check(rc, "map update batch (device)")

    def map_delete_batch(self, m: int, keys):
        """Delete n keys on the device copy; found[n] = the key was present before the call."""
        return self._keyed(m, keys, "map_delete_batch", "map delete batch", values=False)[0]

    # ---- scan and expire on the device copy (ARRAY / HASH; xe_map_scan_device / xe_map_expire_device)
    def _map_scan(self, m: int, flt, cap, on_device: bool, expire: bool):
        what, name = ("map expire", "map_expire") if expire else ("map scan", "map_scan")
        fn = getattr(self.lib, name + ("_device" if on_device else ""))
        cf, fp = self._c_filter(flt)
        n = C.c_uint64(0)
        stream = (None,) if on_device else ()
        return tuple(self._rows(what, n, (self._key_size(m), self.map_defs[m].value_size), cap, on_device,
                                lambda kp, vp, cap: fn(self.h, m, fp, kp, vp, cap, C.byref(n), *stream),
                                lambda: self.lib.map_scan_device(self.h, m, fp, None, None, 0, C.byref(n), None)))

    def map_scan(self, m: int, flt: "MapFilter | None" = None, cap: int | None = None, on_device: bool = False):
        """(keys[r, key_size], values[r, value_size], matched): the entries of the device copy that satisfy
        `flt` (None: all of them), in ascending slot order; r = min(matched, cap). cap None: count first,
        then fetch them all. on_device: CUDA tensors instead of numpy arrays. ARRAY keys are u32 indices."""
        return self._map_scan(m, flt, cap, on_device, False)

    def map_expire(self, m: int, flt: "MapFilter | None" = None, cap: int | None = None, on_device: bool = False):
        """map_scan that also removes the r entries it returns (HASH; xe_map_expire_device)."""
        return self._map_scan(m, flt, cap, on_device, True)

    # ---- in-place edits of value fields on the device copy (xe_map_modify_device / xe_map_modify_batch_device)
    @staticmethod
    def _c_edits(edits):
        edits = list(edits)
        arr = (N.MapEdit * max(len(edits), 1))()
        for i, e in enumerate(edits):
            arr[i] = N.MapEdit(e.op, e.offset, e.width, MM_OPERAND_FIELD if e.operand_field else 0, e.operand)
        return arr, len(edits)

    def map_modify(self, m: int, edits, flt: "MapFilter | None" = None, cap: int | None = None, on_device: bool = False,
                   report: bool = True):
        """(keys[r, key_size], values_before[r, value_size], matched): the `edits` (MapEdit, in list order)
        applied in place to the first r = min(matched, cap) entries of the device copy that satisfy `flt`, in
        map_scan's order; the values are those from before the edits. cap None: every match (counted first, then
        fetched). report False: nothing is reported and only matched is returned. on_device: CUDA tensors."""
        ce, ne = self._c_edits(edits)
        cf, fp = self._c_filter(flt)
        n = C.c_uint64(0)
        if not report:
            if on_device:
                self._synced_device()
            room = (1 << 64) - 1 if cap is None else cap
            self._check(self.lib.map_modify_device(self.h, m, fp, ce, ne, None, None, room, C.byref(n), None), "map modify")
            return int(n.value)
        fn, stream = (self.lib.map_modify_device, (None,)) if on_device else (self.lib.map_modify, ())
        return tuple(self._rows("map modify", n, (self._key_size(m), self.map_defs[m].value_size), cap, on_device,
                                lambda kp, vp, cap: fn(self.h, m, fp, ce, ne, kp, vp, cap, C.byref(n), *stream),
                                lambda: self.lib.map_scan_device(self.h, m, fp, None, None, 0, C.byref(n), None)))

    def map_modify_batch(self, m: int, keys, edits, on_device: bool | None = None):
        """(values_before[n, value_size], found[n]): the `edits` applied in place to the entries of n keys on
        the device copy, once per distinct present key; absent keys are reported and nothing is created.
        on_device None: CUDA tensors for keys give tensors back (xe_map_modify_batch_device), numpy arrays go
        through staging; True / False: the keys are moved to the device / the host first."""
        if on_device is not None and on_device != self._is_dev(keys):
            if on_device:
                import torch
                keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.uint8)).to(torch.device("cuda", self.settings.device))
            else:
                keys = keys.cpu().numpy()
        return self._keyed(m, keys, "map_modify_batch", "map modify batch", pre=self._c_edits(edits))

    # ---- top-K, evict and statistics on the device copy (xe_map_top_device / xe_map_evict_device / xe_map_stats)
    def _map_top(self, m: int, order: "MapOrder", k: int, flt, on_device: bool, ranked: bool, evict: bool):
        d = self.map_defs[m]
        what, name = ("map evict", "map_evict") if evict else ("map top", "map_top")
        fn = getattr(self.lib, name + ("_device" if on_device else ""))
        cf, fp = self._c_filter(flt)
        co = N.MapOrder(order.offset, order.width, int(order.descending), 0)
        n, cut = C.c_uint64(0), C.c_uint64(0)
        stream = (None,) if on_device else ()
        # (r <= matched <= max_entries: no buffer of k entries for a huge k)
        keys, vals, matched = self._rows(what, n, (self._key_size(m), d.value_size), k, on_device,
                                         lambda kp, vp, k: fn(self.h, m, fp, C.byref(co), kp, vp, k, C.byref(n), C.byref(cut), *stream),
                                         rows=min(k, d.max_entries))
        r = len(keys)
        if ranked and r > 1:  # the call reports in slot order: a stable sort on the field keeps the tie order
            if on_device:
                import torch
                f = torch.zeros(r, dtype=torch.int64, device=keys.device)
                for b in range(order.width):
                    f |= vals[:, order.offset + b].to(torch.int64) << (8 * b)
                f ^= torch.tensor(-(1 << 63), dtype=torch.int64, device=keys.device)  # unsigned order through signed compares
                if order.descending:
                    f = ~f
                idx = torch.sort(f, stable=True).indices
            else:
                f = np.zeros(r, dtype=np.uint64)
                for b in range(order.width):
                    f |= vals[:, order.offset + b].astype(np.uint64) << np.uint64(8 * b)
                idx = np.argsort(~f if order.descending else f, kind="stable")
            keys, vals = keys[idx], vals[idx]
        return keys, vals, matched, int(cut.value)

    def map_top(self, m: int, order: "MapOrder", k: int, flt: "MapFilter | None" = None, on_device: bool = False,
                ranked: bool = True):
        """(keys[r], values[r], matched, cut): the r = min(k, matched) entries that rank first by `order`
        among those `flt` selects (equal fields in slot order); cut is the r-th entry's field. ranked: rows
        in rank order; otherwise in the slot order the call reports. on_device: CUDA tensors."""
        return self._map_top(m, order, k, flt, on_device, ranked, False)

    def map_evict(self, m: int, order: "MapOrder", k: int, flt: "MapFilter | None" = None, on_device: bool = False,
                  ranked: bool = True):
        """map_top that also removes the r entries it returns (HASH; xe_map_evict_device)."""
        return self._map_top(m, order, k, flt, on_device, ranked, True)

    def map_stats(self, m: int, field: "MapOrder", flt: "MapFilter | None" = None) -> dict:
        """{count, sum (mod 2^64), min, max} of `field` over the entries `flt` selects (xe_map_stats)."""
        cf, fp = self._c_filter(flt)
        co = N.MapOrder(field.offset, field.width, 0, 0)
        out = N.MapStats()
        self._check(self.lib.map_stats(self.h, m, fp, C.byref(co), C.byref(out), None), "map stats")
        return {"count": out.count, "sum": out.sum, "min": out.min, "max": out.max}

    def map_group(self, src: int, dst: int, group: "MapGroup", flt: "MapFilter | None" = None) -> tuple[int, int]:
        """(matched, created): the entries of map `src` that `flt` selects, folded by `group` into the
        accumulators of map `dst`'s entries on the device (xe_map_group); created: the new HASH entries."""
        cf, fp = self._c_filter(flt)
        cg = N.MapGroup(group.from_, group.offset, group.len, group.measure_off, group.measure_width, group.count_off,
                        group.sum_off, 0)
        n, new = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.map_group(self.h, src, fp, C.byref(cg), dst, C.byref(n), C.byref(new), None), "map group")
        return int(n.value), int(new.value)

    def map_join(self, src: int, other: int, join: "MapJoin", flt: "MapFilter | None" = None, cap: int | None = None,
                 on_device: bool = False, remove: bool = False, other_values: bool = False):
        """(keys[r], values[r][, other_values[r]], matched, selected): the entries of map `src` that `flt` selects
        (selected of them) and whose join key is (MJ_PRESENT) or is not (MJ_ABSENT) an entry of map `other`
        (matched of them), in map_scan's order; r = min(matched, cap). cap None: count first, then fetch them
        all. other_values: also the values of the entries of `other` they joined with (zeros under MJ_ABSENT).
        remove: the r returned entries are removed from `src` (HASH). on_device: CUDA tensors (xe_map_join_device)."""
        cf, fp = self._c_filter(flt)
        cj0 = N.MapJoin(join.from_, join.offset, join.len, join.mode, 0, 0)  # (counting removes nothing)
        cj = N.MapJoin(join.from_, join.offset, join.len, join.mode, MJ_REMOVE if remove else 0, 0)
        n, sel = C.c_uint64(0), C.c_uint64(0)
        fn, stream = (self.lib.map_join_device, (None,)) if on_device else (self.lib.map_join, ())
        widths = [self._key_size(src), self.map_defs[src].value_size] + ([self.map_defs[other].value_size] if other_values else [])

        def call(kp, vp, *rest):
            return fn(self.h, src, fp, C.byref(cj), other, kp, vp, rest[0] if other_values else None, rest[-1], C.byref(n), C.byref(sel),
                      *stream)

        def count():
            return self.lib.map_join_device(self.h, src, fp, C.byref(cj0), other, None, None, None, 0, C.byref(n), C.byref(sel), None)

        return tuple(self._rows("map join", n, widths, cap, on_device, call, count) + [int(sel.value)])

    def map_compact(self, m: int, count_only: bool = False) -> dict:
        """{tombstones, moved, longest_run, via_host}: every tombstone of HASH map `m` removed on the device
        copy, the live entries moved to where linear probing wants them (xe_map_compact). count_only:
        measure and change nothing."""
        info = N.MapCompactInfo()
        self._check(self.lib.map_compact(self.h, m, MC_COUNT_ONLY if count_only else 0, C.byref(info), None), "map compact")
        return {"tombstones": info.tombstones, "moved": info.moved, "longest_run": info.longest_run, "via_host": info.via_host}

    # ---- LRU_HASH maps on the device copy (xe_lru_*): lookup, delete, the usage order and eviction by it
    def lru_lookup_batch(self, m: int, keys, peek: bool = False):
        """(values[n, value_size], found[n]) of n keys of LRU_HASH map `m`, read from the device copy. Without
        `peek` the found keys are promoted as map_lookup key by key in order promotes them."""
        return self._keyed(m, keys, "lru_lookup_batch", "lru lookup batch", post=(LRU_PEEK if peek else 0,))

    def lru_delete_batch(self, m: int, keys):
        """Delete n keys of LRU_HASH map `m` on the device copy; found[n] = the key was present before the call."""
        return self._keyed(m, keys, "lru_delete_batch", "lru delete batch", values=False)[0]

    def _lru_order(self, m: int, k: int, flt, oldest_first: bool, on_device: bool, evict: bool):
        d = self.map_defs[m]
        what, name = ("lru evict", "lru_evict") if evict else ("lru order", "lru_order")
        fn = getattr(self.lib, name + ("_device" if on_device else ""))
        cf, fp = self._c_filter(flt)
        flags = LRU_OLDEST_FIRST if oldest_first else 0
        k = min(int(k), d.max_entries)  # (no more entries than the map holds come back)
        n = C.c_uint64(0)
        stream = (None,) if on_device else ()
        return tuple(self._rows(what, n, (d.key_size, d.value_size), k, on_device,
                                lambda kp, vp, k: fn(self.h, m, fp, flags, kp, vp, k, C.byref(n), *stream)))

    def lru_order(self, m: int, k: int, flt: "MapFilter | None" = None, oldest_first: bool = False, on_device: bool = False):
        """(keys[r, key_size], values[r, value_size], matched): the r = min(k, matched) entries of LRU_HASH map
        `m` whose value satisfies `flt` (None: all) that were used most recently (oldest_first: least recently),
        in that order, read from the device copy. on_device: CUDA tensors instead of numpy arrays."""
        return self._lru_order(m, k, flt, oldest_first, on_device, False)

    def lru_evict(self, m: int, k: int, flt: "MapFilter | None" = None, oldest_first: bool = True, on_device: bool = False):
        """lru_order that also removes the r entries it returns; by default the least recently used, the
        map's own eviction rule applied k times."""
        return self._lru_order(m, k, flt, oldest_first, on_device, True)

    def map_traffic(self, m: int) -> tuple[int, int]:
        """xe_debug_map_traffic: (uploads, downloads) of the whole map so far."""
        up, down = C.c_uint64(), C.c_uint64()
        self._check(self.lib.debug_map_traffic(self.h, m, C.byref(up), C.byref(down)), "map traffic")
        return up.value, down.value

    def map_values_bytes(self, m: int) -> int:
        b = C.c_uint64()
        self._check(self.lib.map_values_bytes(self.h, m, C.byref(b)), "map values bytes")
        return b.value

    # ---- running
    def run_batch(self, umem: np.ndarray, descs: np.ndarray, want_regs: bool = False) -> BatchResult:
        """Host-memory batch (end-to-end form). `umem` (uint8) receives packet writes."""
        d_desc, d_res, d_regs = N.np_dtypes()
        assert umem.dtype == np.uint8 and umem.flags.c_contiguous
        descs = np.ascontiguousarray(descs, dtype=d_desc)
        n = len(descs)
        res = np.zeros(n, dtype=d_res)
        ver = np.zeros(n, dtype=np.uint32)
        regs = np.zeros(n, dtype=d_regs) if want_regs else None
        st = N.BatchStats()
        fn = self.lib.run_batch_host if self.lib.has("run_batch_host") else self.lib.run_batch
        rc = fn(self.h, umem.ctypes.data if umem.size else None, umem.size, descs.ctypes.data if n else None, n,
                res.ctypes.data if n else None, ver.ctypes.data if n else None,
                regs.ctypes.data if (regs is not None and n) else None, C.byref(st))
        self._check(rc, "run batch")
        return BatchResult(res, ver, regs, _stats_dict(st))

    def run_batch_host_ptrs(self, umem: int, umem_len: int, desc: int, n: int, verdicts: int = 0,
                            results: int = 0) -> dict:
        """Host-memory batch over caller-owned (ideally pinned) buffers given as addresses."""
        st = N.BatchStats()
        rc = self.lib.run_batch_host(self.h, umem or None, umem_len, desc or None, n, results or None,
                                     verdicts or None, None, C.byref(st))
        self._check(rc, "run batch (host pointers)")
        return _stats_dict(st)

    def run_batch_device(self, d_umem: int, umem_len: int, d_desc: int, n: int, d_results: int = 0,
                         d_verdicts: int = 0, d_regs: int = 0, stream: int = 0) -> dict:
        """Device-resident batch: all pointers are device addresses (e.g. torch tensor .data_ptr())."""
        st = N.BatchStats()
        rc = self.lib.run_batch_device(self.h, d_umem or None, umem_len, d_desc or None, n, d_results or None,
                                       d_verdicts or None, d_regs or None, stream or None, C.byref(st))
        self._check(rc, "run batch (device)")
        return _stats_dict(st)

    def run_batch_device_async(self, d_umem: int, umem_len: int, d_desc: int, n: int, d_results: int = 0,
                               d_verdicts: int = 0, d_regs: int = 0, stream: int = 0) -> "PendingBatch":
        """Pipelined device-resident batch (xe_run_batch_device_async): queued behind the batches in
        flight on the same stream; the result equals run_batch_device in submission order. The returned
        handle's .stats() completes the pipeline (xe_sync) and gives this batch's statistics."""
        st = N.BatchStats()
        rc = self.lib.run_batch_device_async(self.h, d_umem or None, umem_len, d_desc or None, n, d_results or None,
                                             d_verdicts or None, d_regs or None, stream or None, C.byref(st))
        self._check(rc, "run batch (device, pipelined)")
        pb = PendingBatch(self, st)
        self._pending.append(pb)
        return pb

    def prepare(self) -> None:
        """xe_prepare: compile the per-program kernel (and its keyed variant) for the current program and
        map geometry now instead of in the first batch. Releases the GIL (ctypes), so several VMs can
        prepare from a thread pool and their kernels compile concurrently. No-op on libraries without it."""
        if self.lib.has("prepare"):
            self._check(self.lib.prepare(self.h), "prepare")

    def kernel_sources(self, variants=(0, 1, 2)) -> list[str]:
        """Sources of the per-program kernels xe_prepare would build (0: the kernel, 1: its keyed variant
        when the program may write map entries, 2: its verdict-only variant); [] when the VM runs the
        interpreter."""
        out = []
        for variant in variants:
            n = C.c_size_t()
            rc = self.lib.kernel_source(self.h, variant, None, 0, C.byref(n))
            if rc == -95:  # XE_ERR_UNSUPPORTED
                continue
            self._check(rc, "kernel source")
            buf = C.create_string_buffer(n.value + 1)
            self._check(self.lib.kernel_source(self.h, variant, buf, n.value + 1, C.byref(n)), "kernel source")
            out.append(buf.value.decode())
        return out

    def set_schedule(self, sched: int) -> None:
        """xe_debug_set_schedule: permute the chunk -> wave schedule of later parallel passes (0 = default)."""
        self._check(self.lib.debug_set_schedule(self.h, sched), "set schedule")

    def set_lru_epoch(self, epoch: int) -> None:
        """xe_debug_set_lru_epoch: the run counter of the LRU stamps (tests reach its renumbering)."""
        self._check(self.lib.debug_set_lru_epoch(self.h, epoch), "set LRU epoch")

    def map_pool(self, m: int) -> tuple[int, int]:
        """xe_debug_map_pool: (room, next fresh id) of an ordered map's device value pool."""
        room, nxt = C.c_uint64(), C.c_uint64()
        self._check(self.lib.debug_map_pool(self.h, m, C.byref(room), C.byref(nxt)), "map pool")
        return room.value, nxt.value

    def sync(self) -> None:
        """Complete every pipelined batch (in-order replays included)."""
        rc = self.lib.sync(self.h)
        self._pending.clear()
        self._check(rc, "sync")

    def cancel(self) -> int:
        """xe_cancel (RunContext's cancellation, emulator/vm.go:117-134): drop every pipelined batch not
        completed yet; the maps return to the state before the oldest of them. Returns how many."""
        k = C.c_uint32()
        rc = self.lib.cancel(self.h, C.byref(k))
        self._pending.clear()
        self._check(rc, "cancel")
        return k.value

    # ---- Step / VM.String: per-packet instruction trace
    def trace(self, packets, max_steps: int = 256) -> None:
        """xe_trace_config: record the first max_steps Steps of each listed packet of every batch
        ([] turns it off)."""
        arr = np.ascontiguousarray(np.asarray(list(packets), dtype=np.uint32))
        self._check(self.lib.trace_config(self.h, arr.ctypes.data if len(arr) else None, len(arr),
                                          max_steps if len(arr) else 0), "trace config")

    def trace_read(self, packet: int) -> np.ndarray:
        """The Step records of `packet` in the last batch (N.np_trace_dtype(): pc, pi, sf, kind[11], val[11])."""
        n = C.c_uint32()
        self._check(self.lib.trace_read(self.h, packet, None, 0, C.byref(n)), "trace read")
        out = np.zeros(n.value, dtype=N.np_trace_dtype())
        if n.value:
            self._check(self.lib.trace_read(self.h, packet, out.ctypes.data, n.value, C.byref(n)), "trace read")
        return out

    # ---- the helper table (VM.HelperFunctions)
    def set_helper(self, hid: int, fn) -> None:
        """Replace helper `hid` (emulator/helper_functions.go:17 HelperFunc): fn(packet, args[5], kinds[5])
        returns R0 (an int) or raises to abort the packet (XE_E_HOST_HELPER); fn=None makes the entry nil."""
        if fn is None:
            self._check(self.lib.set_helper(self.h, hid, N.HELPER_FN(), None), "set helper")
            self._helpers.pop(hid, None)
            return

        def tramp(_user, packet, args, kinds, r0):
            try:
                r0[0] = _wrap64(fn(int(packet), [args[i] for i in range(5)], [kinds[i] for i in range(5)]))
                return 0
            except Exception:
                return 1

        cb = N.HELPER_FN(tramp)
        self._check(self.lib.set_helper(self.h, hid, cb, None), "set helper")
        self._helpers[hid] = cb

    def reset_helper(self, hid: int) -> None:
        """Entry `hid` back to LinuxHelperFunctions' (the built-in helper or nil)."""
        self._check(self.lib.reset_helper(self.h, hid), "reset helper")
        self._helpers.pop(hid, None)

    # ---- multi-GPU shard support
    def map_delta(self, m: int, d_out: int, stream: int = 0, lane: int = 0) -> None:
        self._check(self.lib.map_delta(self.h, m, lane, d_out, stream or None), "map delta")

    def map_delta_lane(self, m: int) -> int:
        """Lane width in bytes of map_delta / map_apply_delta (the width of the last run's map adds)."""
        v = C.c_uint32()
        self._check(self.lib.map_delta_lane(self.h, m, C.byref(v)), "map delta lane")
        return v.value

    def map_apply_delta(self, m: int, d_in: int, stream: int = 0, lane: int = 0) -> None:
        self._check(self.lib.map_apply_delta(self.h, m, lane, d_in, stream or None), "map apply delta")

    def epoch_begin(self, stream: int = 0) -> None:
        """xe_epoch_begin: later map deltas / footprints cover every batch from here (a shard epoch)."""
        self._check(self.lib.epoch_begin(self.h, stream or None), "epoch begin")

    def epoch_end(self) -> None:
        self._check(self.lib.epoch_end(self.h), "epoch end")

    def footprint(self) -> np.ndarray:
        """xe_footprint record of the last run (or of the open shard epoch): [flags, (read, add, widths) per map]."""
        nw = C.c_uint32()
        self._check(self.lib.footprint(self.h, None, 0, C.byref(nw)), "footprint")
        out = np.zeros(nw.value, dtype=np.uint64)
        self._check(self.lib.footprint(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), nw.value, C.byref(nw)),
                    "footprint")
        return out

    def shard_check(self, fps: np.ndarray, nshards: int) -> tuple[bool, list[int]]:
        """xe_shard_check over the concatenated footprint records of the shards, in shard order."""
        fps = np.ascontiguousarray(fps, dtype=np.uint64)
        nw = len(fps) // nshards
        lanes = np.zeros(max(1, (nw - 1) // 3), dtype=np.uint32)
        rc = self.lib.shard_check(fps.ctypes.data, nshards, nw, lanes.ctypes.data)
        self._check(rc, "shard check")
        return rc == 1, [int(x) for x in lanes]

    def map_state_bytes(self, m: int) -> int:
        b = C.c_uint64()
        self._check(self.lib.map_state_bytes(self.h, m, C.byref(b)), "map state bytes")
        return b.value

    def map_state_export(self, m: int, d_out: int, stream: int = 0) -> None:
        self._check(self.lib.map_state_export(self.h, m, d_out, stream or None), "map state export")

    def map_state_import(self, m: int, d_in: int, stream: int = 0) -> None:
        self._check(self.lib.map_state_import(self.h, m, d_in, stream or None), "map state import")


class Multi:
    """One process driving N devices (xe_multi_create / xe_run_batch_multi): vms[k] on its own device
    (or sharing one, in tests), set up identically by the caller."""

    def __init__(self, vms: list[VM]):
        self.vms = vms
        self.lib = vms[0].lib
        arr = (C.c_void_p * len(vms))(*[v.h.value for v in vms])
        h = C.c_void_p()
        rc = self.lib.multi_create(arr, len(vms), C.byref(h))
        if rc:
            raise EmulatorError(rc, "multi create")
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.multi_destroy(self.h)
            self.h = None

    def run(self, d_umem: list[int], umem_len: list[int], d_desc: list[int], n: list[int],
            d_results: list[int] | None = None, d_verdicts: list[int] | None = None) -> tuple[list[dict], bool]:
        """Run shard k = (d_umem[k], d_desc[k], n[k]) on vms[k]; maps end equal to the single-VM result."""
        G = len(self.vms)
        ptrs = lambda xs: (C.c_void_p * G)(*[x or None for x in xs])
        sts = (N.BatchStats * G)()
        rep = C.c_uint32()
        rc = self.lib.run_batch_multi(self.h, ptrs(d_umem), (C.c_uint64 * G)(*umem_len), ptrs(d_desc),
                                      (C.c_uint32 * G)(*n), ptrs(d_results) if d_results else None,
                                      ptrs(d_verdicts) if d_verdicts else None, sts, C.byref(rep))
        if rc:
            raise EmulatorError(rc, "run batch multi: " + self.lib.multi_last_error(self.h).decode(errors="replace"))
        return [_stats_dict(s) for s in sts], bool(rep.value)
