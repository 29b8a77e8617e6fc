"""ctypes binding of the C ABI declared in include/xdpemu.h.

The same binding drives three libraries with identical signatures: the product
(gobpfld_amd/libxdpemu.so, prefix ``xe_``), and — in tests only — the CPU oracle
(oracle/liboracle.so, prefix ``orc_``) and the host simulation of the device logic.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PRODUCT_LIB = ROOT / "gobpfld_amd" / "libxdpemu.so"
TUNING_LIB = ROOT / "gobpfld_amd" / "libxdpemu_tuning.so"  # -DXE_TUNING debug build (scripts/ A/B runs)


def product_path() -> Path:
    """The product library, or — only when XE_LIB names it — the tuning build of the same sources
    (`python -m gobpfld_amd.build --tuning`). Nothing else may stand in for the product: XE_LIB naming
    any other file (the host simulation, the oracle, a stray copy) is an error, not a silent swap."""
    import os
    env = os.environ.get("XE_LIB")
    if not env:
        return PRODUCT_LIB
    p = Path(env).resolve()
    if p not in (PRODUCT_LIB.resolve(), TUNING_LIB.resolve()):
        raise RuntimeError(f"XE_LIB={env}: only {PRODUCT_LIB.name} or {TUNING_LIB.name} may serve as the product library")
    return p


class Desc(C.Structure):  # xsk.go:695-701
    _fields_ = [("addr", C.c_uint64), ("len", C.c_uint32), ("options", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_uint8), ("r0_kind", C.c_uint8), ("code", C.c_uint16),
                ("pc", C.c_uint32), ("r0", C.c_int64)]


class Regs(C.Structure):
    _fields_ = [("val", C.c_int64 * 10), ("kind", C.c_uint8 * 10), ("region", C.c_uint8 * 10),
                ("map", C.c_uint8 * 10), ("pad", C.c_uint8 * 2), ("steps", C.c_uint32)]


class MapDef(C.Structure):  # map_definition.go:15-27
    _fields_ = [("type", C.c_uint32), ("key_size", C.c_uint32), ("value_size", C.c_uint32),
                ("max_entries", C.c_uint32), ("flags", C.c_uint32)]


class Settings(C.Structure):  # emulator/vm.go:282-296 + device knobs
    _fields_ = [("stack_frame_size", C.c_int32), ("max_stack_frames", C.c_int32),
                ("max_steps", C.c_uint64), ("ingress_ifindex", C.c_uint32),
                ("rx_queue_index", C.c_uint32), ("device", C.c_int32), ("mode", C.c_uint32),
                ("engine", C.c_uint32)]


class PcapInfo(C.Structure):  # include/xdpemu_io.h
    _fields_ = [("linktype", C.c_uint32), ("snaplen", C.c_uint32), ("nanosecond", C.c_uint32),
                ("swapped", C.c_uint32), ("first_record", C.c_uint64)]


class DispatchCounts(C.Structure):  # xe_dispatch_counts (include/xdpemu_io.h)
    _fields_ = [("offset", C.c_uint32 * 6), ("invalid", C.c_uint32), ("failed", C.c_uint32)]


class TraceRec(C.Structure):  # xe_trace_rec: one Step's VM.String (emulator/vm.go:248-270)
    _fields_ = [("packet", C.c_uint32), ("step", C.c_uint32), ("pc", C.c_int32), ("pi", C.c_int32),
                ("sf", C.c_uint32), ("kind", C.c_uint8 * 11), ("pad", C.c_uint8), ("val", C.c_int64 * 11)]


class MapFilter(C.Structure):  # xe_map_filter
    _fields_ = [("op", C.c_uint32), ("offset", C.c_uint32), ("width", C.c_uint32), ("pad", C.c_uint32),
                ("operand", C.c_uint64)]


class MapOrder(C.Structure):  # xe_map_order
    _fields_ = [("offset", C.c_uint32), ("width", C.c_uint32), ("descending", C.c_uint32), ("pad", C.c_uint32)]


class MapStats(C.Structure):  # struct xe_map_stats
    _fields_ = [("count", C.c_uint64), ("sum", C.c_uint64), ("min", C.c_uint64), ("max", C.c_uint64)]


class MapGroup(C.Structure):  # xe_map_group_spec
    _fields_ = [("from_", C.c_uint32), ("offset", C.c_uint32), ("len", C.c_uint32), ("measure_off", C.c_uint32),
                ("measure_width", C.c_uint32), ("count_off", C.c_uint32), ("sum_off", C.c_uint32), ("pad", C.c_uint32)]


class MapJoin(C.Structure):  # xe_map_join_spec
    _fields_ = [("from_", C.c_uint32), ("offset", C.c_uint32), ("len", C.c_uint32), ("mode", C.c_uint32),
                ("flags", C.c_uint32), ("pad", C.c_uint32)]


class MapEdit(C.Structure):  # xe_map_edit
    _fields_ = [("op", C.c_uint32), ("offset", C.c_uint32), ("width", C.c_uint32), ("flags", C.c_uint32),
                ("operand", C.c_uint64)]


class MapCompactInfo(C.Structure):  # xe_map_compact_info
    _fields_ = [("tombstones", C.c_uint64), ("moved", C.c_uint64), ("longest_run", C.c_uint32), ("via_host", C.c_uint32)]


# xe_helper_fn: int fn(void* user, uint32_t packet, const int64_t args[5], const uint8_t kinds[5], int64_t* r0)
HELPER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8),
                        C.POINTER(C.c_int64))


class BatchStats(C.Structure):
    _fields_ = [("packets", C.c_uint64), ("steps", C.c_uint64), ("status_count", C.c_uint64 * 8),
                ("mode_used", C.c_uint32), ("conflict", C.c_uint32), ("kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("engine_used", C.c_uint32), ("grid_blocks", C.c_uint32)]


# numpy dtypes matching the structs (for zero-copy batch buffers)
def np_dtypes():
    import numpy as np
    desc = np.dtype([("addr", "<u8"), ("len", "<u4"), ("options", "<u4")])
    result = np.dtype([("status", "u1"), ("r0_kind", "u1"), ("code", "<u2"), ("pc", "<u4"), ("r0", "<i8")])
    regs = np.dtype([("val", "<i8", (10,)), ("kind", "u1", (10,)), ("region", "u1", (10,)),
                     ("map", "u1", (10,)), ("pad", "u1", (2,)), ("steps", "<u4")], align=True)
    assert desc.itemsize == 16 and result.itemsize == 16 and regs.itemsize == C.sizeof(Regs)
    return desc, result, regs


def np_trace_dtype():
    import numpy as np
    t = np.dtype([("packet", "<u4"), ("step", "<u4"), ("pc", "<i4"), ("pi", "<i4"), ("sf", "<u4"),
                  ("kind", "u1", (11,)), ("pad", "u1"), ("val", "<i8", (11,))], align=True)
    assert t.itemsize == C.sizeof(TraceRec) == 120
    return t


P = C.c_void_p
_SIGS = {
    "default_settings": (C.c_int, [P]),
    "create": (C.c_int, [P, C.POINTER(P)]),
    "destroy": (None, [P]),
    "last_error": (C.c_char_p, [P]),
    "add_raw_program": (C.c_int, [P, P, C.c_uint32, C.POINTER(C.c_int32)]),
    "set_entrypoint": (C.c_int, [P, C.c_int32]),
    "add_map": (C.c_int, [P, P, P, C.c_size_t, C.POINTER(C.c_int32)]),
    "map_lookup": (C.c_int, [P, C.c_int32, P, P]),
    "map_update": (C.c_int, [P, C.c_int32, P, P]),
    "map_delete": (C.c_int, [P, C.c_int32, P]),
    "map_update_batch": (C.c_int, [P, C.c_int32, P, P, C.c_uint64]),
    "map_count": (C.c_int, [P, C.c_int32, C.POINTER(C.c_uint64)]),
    "map_dump": (C.c_int, [P, C.c_int32, P, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "map_dump_list": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "map_lru_order": (C.c_int, [P, C.c_int32, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "map_push": (C.c_int, [P, C.c_int32, P]),
    "run_batch": (C.c_int, [P, P, C.c_uint64, P, C.c_uint32, P, P, P, P]),  # oracle form
    "run_batch_host": (C.c_int, [P, P, C.c_uint64, P, C.c_uint32, P, P, P, P]),
    "run_batch_device": (C.c_int, [P, P, C.c_uint64, P, C.c_uint32, P, P, P, P, P]),
    "run_batch_device_async": (C.c_int, [P, P, C.c_uint64, P, C.c_uint32, P, P, P, P, P]),
    "sync": (C.c_int, [P]),
    "cancel": (C.c_int, [P, C.POINTER(C.c_uint32)]),
    "trace_config": (C.c_int, [P, P, C.c_uint32, C.c_uint32]),
    "trace_read": (C.c_int, [P, C.c_uint32, P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "set_helper": (C.c_int, [P, C.c_uint32, HELPER_FN, P]),
    "reset_helper": (C.c_int, [P, C.c_uint32]),
    "prepare": (C.c_int, [P]),
    "debug_set_schedule": (C.c_int, [P, C.c_uint32]),
    "debug_set_lru_epoch": (C.c_int, [P, C.c_uint64]),
    "debug_map_pool": (C.c_int, [P, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "set_kernel_cache": (C.c_int, [C.c_char_p]),
    "kernel_source": (C.c_int, [P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "compile_kernel_source": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "kernel_object_name": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "kernel_cache_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "map_values_bytes": (C.c_int, [P, C.c_int32, C.POINTER(C.c_uint64)]),
    "map_delta": (C.c_int, [P, C.c_int32, C.c_uint32, P, P]),
    "map_apply_delta": (C.c_int, [P, C.c_int32, C.c_uint32, P, P]),
    "map_delta_lane": (C.c_int, [P, C.c_int32, C.POINTER(C.c_uint32)]),
    "footprint": (C.c_int, [P, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "shard_check": (C.c_int, [P, C.c_uint32, C.c_uint32, P]),
    "epoch_begin": (C.c_int, [P, P]),
    "epoch_end": (C.c_int, [P]),
    "map_state_bytes": (C.c_int, [P, C.c_int32, C.POINTER(C.c_uint64)]),
    "map_state_export": (C.c_int, [P, C.c_int32, P, P]),
    "map_state_import": (C.c_int, [P, C.c_int32, P, P]),
    "map_lookup_batch_device": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, P, P]),
    "map_update_batch_device": (C.c_int, [P, C.c_int32, P, P, C.c_uint64, P]),
    "map_delete_batch_device": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, P]),
    "map_lookup_batch": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, P]),
    "map_update_batch_staged": (C.c_int, [P, C.c_int32, P, P, C.c_uint64]),
    "map_delete_batch": (C.c_int, [P, C.c_int32, P, C.c_uint64, P]),
    "map_scan_device": (C.c_int, [P, C.c_int32, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), P]),
    "map_expire_device": (C.c_int, [P, C.c_int32, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), P]),
    "map_scan": (C.c_int, [P, C.c_int32, P, P, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "map_expire": (C.c_int, [P, C.c_int32, P, P, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "map_top_device": (C.c_int, [P, C.c_int32, P, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), P]),
    "map_evict_device": (C.c_int, [P, C.c_int32, P, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), P]),
    "map_top": (C.c_int, [P, C.c_int32, P, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "map_evict": (C.c_int, [P, C.c_int32, P, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "map_stats": (C.c_int, [P, C.c_int32, P, P, P, P]),
    "map_group": (C.c_int, [P, C.c_int32, P, P, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), P]),
    "map_join_device": (C.c_int, [P, C.c_int32, P, P, C.c_int32, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), P]),
    "map_join": (C.c_int, [P, C.c_int32, P, P, C.c_int32, P, P, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "map_compact": (C.c_int, [P, C.c_int32, C.c_uint32, P, P]),
    "map_modify_device": (C.c_int, [P, C.c_int32, P, P, C.c_uint32, P, P, C.c_uint64, C.POINTER(C.c_uint64), P]),
    "map_modify": (C.c_int, [P, C.c_int32, P, P, C.c_uint32, P, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "map_modify_batch_device": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, C.c_uint32, P, P, P]),
    "map_modify_batch": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, C.c_uint32, P, P]),
    "debug_map_traffic": (C.c_int, [P, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lru_lookup_batch_device": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, P, C.c_uint32, P]),
    "lru_delete_batch_device": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, P]),
    "lru_order_device": (C.c_int, [P, C.c_int32, P, C.c_uint32, P, P, C.c_uint64, C.POINTER(C.c_uint64), P]),
    "lru_evict_device": (C.c_int, [P, C.c_int32, P, C.c_uint32, P, P, C.c_uint64, C.POINTER(C.c_uint64), P]),
    "lru_lookup_batch": (C.c_int, [P, C.c_int32, P, C.c_uint64, P, P, C.c_uint32]),
    "lru_delete_batch": (C.c_int, [P, C.c_int32, P, C.c_uint64, P]),
    "lru_order": (C.c_int, [P, C.c_int32, P, C.c_uint32, P, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "lru_evict": (C.c_int, [P, C.c_int32, P, C.c_uint32, P, P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "multi_create": (C.c_int, [P, C.c_uint32, C.POINTER(P)]),
    "multi_destroy": (None, [P]),
    "multi_last_error": (C.c_char_p, [P]),
    "run_batch_multi": (C.c_int, [P, P, P, P, P, P, P, P, P]),
    "version": (C.c_char_p, []),
    "device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "decode_names": (C.c_int, [P, C.c_uint32, C.c_char_p, C.c_size_t]),
    # include/xdpemu_io.h
    "pcap_header": (C.c_int, [P, C.c_uint64, P]),
    "pcap_count": (C.c_int, [P, C.c_uint64, P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcap_fill": (C.c_int, [P, C.c_uint64, P, C.POINTER(C.c_uint64), P, C.c_uint64, C.c_uint32, C.c_uint32, P,
                            C.c_uint64, C.c_uint32, P, P, P, C.POINTER(C.c_uint32)]),
    "pcap_pack": (C.c_int, [P, C.c_uint64, P, C.POINTER(C.c_uint64), P, C.c_uint64, C.c_uint32, C.c_uint32,
                            C.c_uint32, P, P, P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "dispatch_scratch_bytes": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint64)]),
    "dispatch_device": (C.c_int, [P, P, P, C.c_uint32, P, P, P, P, C.c_uint64, P]),
    "gather_device": (C.c_int, [P, C.c_uint64, P, P, C.c_uint32, C.c_uint32, P, C.c_uint32, P, C.c_uint64, P, P, P]),
}

# every symbol include/xdpemu.h declares (checked by tests/test_abi.py)
HEADER_SYMBOLS = [
    "xe_default_settings", "xe_create", "xe_destroy", "xe_last_error", "xe_add_raw_program",
    "xe_set_entrypoint", "xe_add_map", "xe_map_lookup", "xe_map_update", "xe_map_delete",
    "xe_map_count", "xe_map_dump", "xe_map_dump_list", "xe_map_lru_order", "xe_map_push", "xe_map_update_batch", "xe_run_batch_device", "xe_run_batch_host",
    "xe_run_batch_device_async", "xe_sync", "xe_prepare", "xe_map_values_bytes", "xe_map_delta", "xe_map_apply_delta", "xe_map_delta_lane", "xe_footprint", "xe_version",
    "xe_device_count", "xe_shard_check", "xe_epoch_begin", "xe_epoch_end", "xe_map_state_bytes", "xe_map_state_export",
    "xe_map_state_import",
    "xe_multi_create", "xe_multi_destroy", "xe_run_batch_multi", "xe_multi_last_error", "xe_debug_set_schedule",
    "xe_debug_set_lru_epoch", "xe_debug_map_pool",
    "xe_map_lookup_batch_device", "xe_map_update_batch_device", "xe_map_delete_batch_device",
    "xe_map_lookup_batch", "xe_map_update_batch_staged", "xe_map_delete_batch", "xe_debug_map_traffic",
    "xe_map_scan_device", "xe_map_expire_device", "xe_map_scan", "xe_map_expire",
    "xe_map_top_device", "xe_map_evict_device", "xe_map_top", "xe_map_evict", "xe_map_stats",
    "xe_map_group", "xe_map_join_device", "xe_map_join", "xe_map_compact",
    "xe_map_modify_device", "xe_map_modify", "xe_map_modify_batch_device", "xe_map_modify_batch",
    "xe_lru_lookup_batch_device", "xe_lru_delete_batch_device", "xe_lru_order_device", "xe_lru_evict_device",
    "xe_lru_lookup_batch", "xe_lru_delete_batch", "xe_lru_order", "xe_lru_evict",
    "xe_set_kernel_cache", "xe_kernel_source", "xe_compile_kernel_source", "xe_kernel_object_name",
    "xe_kernel_cache_stats",
    "xe_cancel", "xe_trace_config", "xe_trace_read", "xe_set_helper", "xe_reset_helper",
]
IO_HEADER_SYMBOLS = ["xe_pcap_header", "xe_pcap_count", "xe_pcap_fill", "xe_pcap_pack",  # include/xdpemu_io.h
                     "xe_dispatch_scratch_bytes", "xe_dispatch_device", "xe_gather_device"]
# the output side of include/xdpemu_io.h
ACT_ABORTED, ACT_DROP, ACT_PASS, ACT_TX, ACT_REDIRECT, ACT_COUNT = 0, 1, 2, 3, 4, 5
XE_DISPATCH_TILE = 2048


class Lib:
    """A loaded emulator library exposing the xdpemu.h calls without their prefix."""

    def __init__(self, path: Path | str, prefix: str = "xe_"):
        self.path = Path(path)
        if not self.path.exists():
            raise FileNotFoundError(
                f"{self.path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        self.dll = C.CDLL(str(self.path))
        self.prefix = prefix
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.dll, prefix + name, None)
            if fn is None:
                continue
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def has(self, name: str) -> bool:
        return hasattr(self, name)


_product: Lib | None = None


def product() -> Lib:
    """The HIP product library. Raises if it is not built — there is no CPU fallback."""
    global _product
    if _product is None:
        try:  # torch bundles its own HIP runtime: have it loaded first so the process holds one
            import torch  # noqa: F401
        except ImportError:
            pass
        _product = Lib(product_path(), "xe_")
        # the package's ahead-of-time kernel cache (gobpfld_amd/aot.py), when it was built
        kdir = ROOT / "gobpfld_amd" / "kernels"
        if kdir.is_dir() and _product.has("set_kernel_cache"):
            _product.set_kernel_cache(str(kdir).encode())
    return _product
