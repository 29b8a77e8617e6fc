#!/usr/bin/env python3
"""Time the device-side group-by (xe_map_group) on C5's flow table (BASELINE configs[4]: HASH, 16-byte keys
and values, 1,048,576 entries, full), after a C5 batch has made the device copy the newer one, beside today's
route to the same answer, measured in the same run.

    python scripts/prof_mapgroup.py --out profiles/mapops/mapgroup.json
    python scripts/prof_mapgroup.py --lib gobpfld_amd/libxdpemu_tuning.so --only-b b_protocol_leaders_0 \
        --out profiles/mapops/mapgroup.json      # adds variant (b) of another build to the file

Variants (the key of C5 is {saddr, daddr, sport, dport, proto, pad}; the value {packets, bytes}):
  (a) by the 4-byte source address (key bytes 0 .. 3) into a HASH map of 2^20 entries, flows and packets per
      source: high cardinality, bound by claims and probes;
  (b) by the protocol byte (key byte 12) into ARRAY(256): two hot groups, bound by the atomics. Run once with
      the product library (wave combining, kMgLeaders = 4) and once with a tuning library built with
      -DXE_MG_LEADERS=0 (every lane adds singly);
  (c) (a) followed by xe_map_top of 1,024 over the result: the top talkers by source.
Before any timing every variant's answer is compared with a whole-table xe_map_scan_device aggregated by numpy.

Calls: device events around single calls on one stream, after warm-up; each call ends with its own stream
synchronisation. The destination is cleared outside the timed region between repetitions (xe_map_expire_device
of everything: the groups then take their old records again; the ARRAY is overwritten with zeros).

One condition is recorded under "acceptance": xe_map_group for (a) must take less wall-clock time than
today's route, xe_map_scan of every entry into host memory followed by a numpy group-by.

The kernels' rows of profiles/mapops/kernel_stats.csv come from a run of this script of their own under
`rocprofv3 --kernel-trace --stats` (the xe_mapgroup_* lines of its kernel statistics, appended)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DST_MAX = 1 << 20


def setup(vm):
    """C5's VM with the two destinations behind its maps. Returns (flow table, per-source HASH, histogram ARRAY)."""
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import MAP_ARRAY, MAP_HASH, MapDef
    W.setup_vm(vm, "c5")
    return 1, vm.add_map(MapDef(MAP_HASH, 4, 16, DST_MAX)), vm.add_map(MapDef(MAP_ARRAY, 4, 16, 256))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4 * 1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--lib", default="", help="another build of the library (the tuning build)")
    ap.add_argument("--only-b", default="", help="time variant (b) alone and add it to --out under this name")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_mapgroup: no GPU")
    from gobpfld_amd import _native as N
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import MG_KEY, MG_NONE, VM, Settings

    vm = VM(Settings(), lib=N.Lib(Path(a.lib).resolve(), "xe_")) if a.lib else VM(Settings())
    m, by_src, hist = setup(vm)
    lib = vm.lib
    n = a.packets
    umem, descs = W.build_batch("c5", 0, n)
    d_umem = torch.from_numpy(umem).cuda()
    d_desc = torch.from_numpy(descs.view(np.uint8)).cuda()
    d_ver = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for _ in range(2):  # (the first loads or compiles the kernel and uploads the table)
        torch.cuda.synchronize()
        vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_verdicts=d_ver.data_ptr(), stream=s)
        torch.cuda.synchronize()
    entries = len(W.c5_map_entries()[0])
    d_keys = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_vals = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_idx = torch.arange(256, dtype=torch.int32, device="cuda").view(torch.uint8).reshape(256, 4)
    d_zero = torch.zeros((256, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def scan(mi: int, cap: int, dk=d_keys, dv=d_vals) -> int:
        cnt = C.c_uint64()
        rc = lib.map_scan_device(vm.h, mi, None, dk.data_ptr() if cap else None, dv.data_ptr() if cap else None, cap, C.byref(cnt), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value

    g_src = N.MapGroup(MG_KEY, 0, 4, 0, 8, 0, 8, 0)    # count at +0, packets at +8
    g_proto = N.MapGroup(MG_KEY, 12, 1, 0, 8, 0, 8, 0)

    def group(g, dst: int) -> tuple[int, int]:
        cnt, new = C.c_uint64(), C.c_uint64()
        rc = lib.map_group(vm.h, m, None, C.byref(g), dst, C.byref(cnt), C.byref(new), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value, new.value

    def top_sources():
        order, cnt, cut = N.MapOrder(8, 8, 1, 0), C.c_uint64(), C.c_uint64()
        rc = lib.map_top_device(vm.h, by_src, None, C.byref(order), d_keys.data_ptr(), d_vals.data_ptr(), 1024, C.byref(cnt), C.byref(cut), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value, cut.value

    def clear_src() -> None:
        cnt = C.c_uint64()
        assert lib.map_expire_device(vm.h, by_src, None, None, None, 1 << 40, C.byref(cnt), s) == 0, lib.last_error(vm.h)

    def clear_hist() -> None:
        assert lib.map_update_batch_device(vm.h, hist, d_idx.data_ptr(), d_zero.data_ptr(), 256, s) == 0, lib.last_error(vm.h)

    # ---- the answers, before any timing: against a whole-table scan aggregated by numpy
    traffic0 = vm.map_traffic(m)
    assert scan(m, entries) == entries
    all_k, all_v = d_keys.cpu().numpy().copy(), d_vals.cpu().numpy().copy()
    packets = all_v.view(np.uint64)[:, 0].copy()

    def aggregate(col: np.ndarray):
        u, inv, cnt = np.unique(col, return_inverse=True, return_counts=True)
        sums = np.zeros(len(u), dtype=np.uint64)
        np.add.at(sums, inv, packets)
        return u, cnt.astype(np.uint64), sums

    saddr = np.ascontiguousarray(all_k[:, 0:4]).view(np.uint32).reshape(-1)
    su, sc, ss = aggregate(saddr)
    pu, pc, ps = aggregate(all_k[:, 12])
    assert group(g_proto, hist) == (entries, 0)
    assert scan(hist, 256) == 256
    hv = d_vals[:256].cpu().numpy().view(np.uint64).reshape(256, 2)
    want = np.zeros((256, 2), dtype=np.uint64)
    want[pu, 0], want[pu, 1] = pc, ps
    assert np.array_equal(hv, want), "variant (b) differs from the numpy aggregate"
    clear_hist()
    if not a.only_b:
        assert group(g_src, by_src) == (entries, len(su))
        assert scan(by_src, entries) == len(su)
        gk = d_keys.reshape(-1)[:len(su) * 4].cpu().numpy().view(np.uint32)  # (4-byte keys, back to back)
        gv = d_vals[:len(su)].cpu().numpy().view(np.uint64).reshape(-1, 2)
        o = np.argsort(gk)
        assert np.array_equal(gk[o], su) and np.array_equal(gv[o, 0], sc) and np.array_equal(gv[o, 1], ss), "variant (a) differs"
        matched, cut = top_sources()
        assert matched == len(su) and cut == int(np.sort(ss)[-1024]), "variant (c) differs"
        clear_src()
        assert group(g_src, by_src) == (entries, len(su)), "the groups did not take their old records"
        clear_src()
    assert vm.map_traffic(m) == traffic0, "a group call moved the whole map"

    def timed(fn) -> tuple[float, float]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), wall

    def a_then_top() -> None:
        group(g_src, by_src)
        top_sources()

    calls = {"b_protocol_array256": (lambda: group(g_proto, hist), clear_hist, int(len(pu)))}
    if a.only_b:
        calls = {a.only_b: calls["b_protocol_array256"]}
    else:
        calls["a_source_hash"] = (lambda: group(g_src, by_src), clear_src, int(len(su)))
        calls["c_source_then_top_1024"] = (a_then_top, clear_src, int(len(su)))
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):
        for k, (fn, clear, _) in calls.items():
            t = timed(fn)
            clear()  # outside the timed region
            if rep >= 3:
                times[k].append(t)
    res = {}
    for k, v in times.items():
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        res[k] = {"calls": len(v), "groups": calls[k][2], "median_ms": float(np.median(ev)), "min_ms": float(min(ev)),
                  "p90_ms": float(np.percentile(ev, 90)), "wall_median_ms": float(np.median(wall))}

    if a.only_b:
        out = json.loads(Path(a.out).read_text())
        out["calls"].update(res)
    else:
        out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": entries, "slots": 2 * W.C5_MAX},
               "batch_packets": n, "sources": int(len(su)), "protocols": int(len(pu)), "calls": res}
        # ---- today's route to (a): xe_map_scan of every entry into host memory, then a numpy group-by
        hk, hvv = np.zeros((entries, 16), np.uint8), np.zeros((entries, 16), np.uint8)
        today, device = [], []
        for rep in range(3 + a.reps):
            cnt = C.c_uint64()
            t0 = time.perf_counter()
            assert lib.map_scan(vm.h, m, None, hk.ctypes.data, hvv.ctypes.data, entries, C.byref(cnt)) == 0
            col = np.ascontiguousarray(hk[:, 0:4]).view(np.uint32).reshape(-1)
            u, inv, c = np.unique(col, return_inverse=True, return_counts=True)
            tot = np.bincount(inv, weights=None, minlength=len(u))  # the counts again, as a host aggregate would
            sums = np.zeros(len(u), dtype=np.uint64)
            np.add.at(sums, inv, hvv.view(np.uint64)[:, 0])
            t1 = time.perf_counter()
            group(g_src, by_src)
            t2 = time.perf_counter()
            clear_src()
            if rep >= 3:
                today.append((t1 - t0) * 1e3)
                device.append((t2 - t1) * 1e3)
        assert np.array_equal(u, su) and np.array_equal(sums, ss) and np.array_equal(tot.astype(np.uint64), sc)
        t_old, t_new = float(np.median(today)), float(np.median(device))
        out["today"] = {"what": "xe_map_scan of every entry into host memory + numpy group-by (wall), beside xe_map_group for (a) (wall)",
                        "calls": len(today), "scan_to_host_then_numpy_median_ms": t_old, "map_group_median_ms": t_new}
        out["acceptance"] = {"today_ms": t_old, "map_group_ms": t_new, "today_over_map_group": t_old / t_new, "faster": t_new < t_old}
        out["whole_map_traffic"] = dict(zip(("uploads", "downloads"), vm.map_traffic(m)))
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
