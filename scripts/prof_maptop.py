#!/usr/bin/env python3
"""Time the device-side top-K, evict and value statistics (xe_map_top_device / xe_map_evict_device /
xe_map_stats) on C5's flow table (BASELINE configs[4]: HASH, 16-byte keys and values, 1,048,576 entries,
full), after a C5 batch has made the device copy the newer one, beside the calls they are built from and
beside today's route to the same answer, all measured in the same run.

    python scripts/prof_maptop.py --out profiles/mapops/maptop.json

The values of C5 are {packets, bytes} counters. As in scripts/prof_mapscan.py, 1,024 entries get bit 41 of
the packet count set before anything is timed, so `ANYBITS 1 << 41` selects exactly those (the count-only
scan the bound below is stated against) and they are the 1,024 largest 8-byte packet counts. The 4-byte
order field is the low half of the packet count. Before any timing every variant's answer is compared with
a whole-table xe_map_scan_device ranked by numpy (lexsort on field and slot position).

Calls: device events around single calls on one stream, after warm-up, the variants taking turns; each call
ends with its own stream synchronisation, so the event time is what the caller waits for. The evict removes
65,536 entries each time; they are installed again (same keys, same values: each takes its old record)
outside the timed region.

Two conditions are recorded under "acceptance":
  * structure: every step of a top call reads the table at most once, so top_1024 on a w-byte field must
    cost no more than (w + 2) x the count-only filtered scan's median;
  * against today's route: xe_map_top (host pointers) of 1,024 must beat xe_map_scan of every entry into
    host memory followed by numpy.argpartition on the field (wall clock, both).
A whole-table device scan followed by torch.topk on the device is recorded for information.
"""
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

MARK = 1 << 41
N_MARK, N_EVICT = 1024, 65536
KS = (1, 1024, 65536)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4 * 1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_maptop: no GPU")
    from gobpfld_amd import _native as N
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import MF_ALL, MF_ANYBITS, VM, Settings

    vm = VM(Settings())
    W.setup_vm(vm, "c5")
    m, lib = 1, vm.lib
    n = a.packets
    umem, descs = W.build_batch("c5", 0, n)
    d_umem = torch.from_numpy(umem).cuda()
    d_desc = torch.from_numpy(descs.view(np.uint8)).cuda()
    d_ver = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def batch() -> None:
        torch.cuda.synchronize()
        vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_verdicts=d_ver.data_ptr(), stream=s)
        torch.cuda.synchronize()

    for _ in range(3):
        batch()  # (the first compiles the kernel and uploads the table)

    keys, _ = W.c5_map_entries()
    entries = len(keys)
    rng = np.random.default_rng(7)
    k_mark = np.ascontiguousarray(keys[rng.permutation(entries)[:N_MARK]])
    v_mark = np.zeros((N_MARK, 2), dtype=np.uint64)
    v_mark[:, 0] = np.uint64(MARK) + np.arange(N_MARK, dtype=np.uint64)
    v_mark[:, 1] = 64
    d_kmark, d_vmark = torch.from_numpy(k_mark).cuda(), torch.from_numpy(v_mark.view(np.uint8).reshape(N_MARK, 16)).cuda()
    d_keys = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_vals = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_kev = torch.empty((N_EVICT, 16), dtype=torch.uint8, device="cuda")
    d_vev = torch.empty((N_EVICT, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def install(d_k, d_v) -> None:
        rc = lib.map_update_batch_device(vm.h, m, d_k.data_ptr(), d_v.data_ptr(), len(d_k), s)
        assert rc == 0, (rc, lib.last_error(vm.h))

    f_all = N.MapFilter(MF_ALL, 0, 0, 0, 0)
    f_mark = N.MapFilter(MF_ANYBITS, 0, 8, 0, MARK)

    def scan(flt, cap: int, out: bool = True) -> int:
        cnt = C.c_uint64()
        rc = lib.map_scan_device(vm.h, m, C.byref(flt), d_keys.data_ptr() if out else None, d_vals.data_ptr() if out else None, cap,
                                 C.byref(cnt), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value

    def top(width: int, desc: bool, k: int, dk=d_keys, dv=d_vals, evict: bool = False):
        order = N.MapOrder(0, width, int(desc), 0)
        cnt, cut = C.c_uint64(), C.c_uint64()
        fn = lib.map_evict_device if evict else lib.map_top_device
        rc = fn(vm.h, m, None, C.byref(order), dk.data_ptr(), dv.data_ptr(), k, C.byref(cnt), C.byref(cut), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value, cut.value

    def stats(width: int) -> dict:
        field, st = N.MapOrder(0, width, 0, 0), N.MapStats()
        rc = lib.map_stats(vm.h, m, None, C.byref(field), C.byref(st), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return {"count": st.count, "sum": st.sum, "min": st.min, "max": st.max}

    install(d_kmark, d_vmark)
    traffic0 = vm.map_traffic(m)

    # ---- what the calls report, before any timing: against a whole-table scan ranked by numpy
    assert scan(f_all, entries) == entries
    all_k, all_v = d_keys.cpu().numpy().copy(), d_vals.cpu().numpy().copy()  # in slot order
    packets = all_v.view(np.uint64)[:, 0].copy()
    pos = np.arange(entries)

    def expected(width: int, desc: bool, k: int):
        f = packets if width == 8 else packets & np.uint64(0xffffffff)
        rank = np.lexsort((pos, ~f if desc else f))[:k]
        return np.sort(rank), int(f[rank[-1]])

    for width in (4, 8):
        for k in KS:
            want, cut = expected(width, True, k)
            assert top(width, True, k) == (entries, cut), (width, k)
            assert np.array_equal(d_keys[:k].cpu().numpy(), all_k[want]) and np.array_equal(d_vals[:k].cpu().numpy(), all_v[want])
    assert top(8, True, N_MARK)[0] == entries  # the marked entries are the 1,024 largest packet counts
    assert set(map(bytes, d_keys[:N_MARK].cpu().numpy())) == set(map(bytes, k_mark))
    for width in (4, 8):
        f = [int(x) for x in (packets if width == 8 else packets & np.uint64(0xffffffff))]
        assert stats(width) == {"count": entries, "sum": sum(f) & ((1 << 64) - 1), "min": min(f), "max": max(f)}
    want, cut = expected(8, False, N_EVICT)
    assert top(8, False, N_EVICT, d_kev, d_vev, evict=True) == (entries, cut)
    assert np.array_equal(d_kev.cpu().numpy(), all_k[want]) and np.array_equal(d_vev.cpu().numpy(), all_v[want])
    assert scan(f_all, 0, out=False) == entries - N_EVICT
    install(d_kev, d_vev)
    assert scan(f_all, entries) == entries
    assert np.array_equal(d_keys.cpu().numpy(), all_k) and np.array_equal(d_vals.cpu().numpy(), all_v), "an evicted key did not take its old record"
    assert vm.map_traffic(m) == traffic0, "a top, an evict or a stats call moved the whole map"

    out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": entries, "slots": 2 * W.C5_MAX},
           "batch_packets": n, "order_fields": {"w4": "the low 4 bytes of the packet count", "w8": "the packet count"},
           "calls": {}, "today": {}}

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

    def evict_once() -> None:
        assert top(8, False, N_EVICT, d_kev, d_vev, evict=True)[0] == entries

    def scan_topk() -> None:  # for information: every entry to device buffers, then torch.topk on the device
        scan(f_all, entries)
        f = d_vals.view(torch.int64)[:, 0]  # (packet counts stay far below 2^63)
        torch.topk(f, 1024).indices.cpu()

    calls = {
        "count_only_filtered": (lambda: scan(f_mark, 0, out=False), N_MARK),
        "scan_all": (lambda: scan(f_all, entries), entries),
        "stats_w8": (lambda: stats(8), entries),
        f"evict_{N_EVICT}_w8": (evict_once, N_EVICT),
        "scan_all_then_torch_topk_1024": (scan_topk, 1024),
    }
    for width in (4, 8):
        for k in KS:
            calls[f"top_{k}_w{width}"] = ((lambda w=width, kk=k: top(w, True, kk)), k)
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):  # three rounds of warm-up, then the variants take turns
        for k, (fn, _) in calls.items():
            t = timed(fn)
            if k.startswith("evict"):
                install(d_kev, d_vev)  # outside the timed region
            if rep >= 3:
                times[k].append(t)
    assert scan(f_all, 0, out=False) == entries
    for k, v in times.items():
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        out["calls"][k] = {"calls": len(v), "selected": calls[k][1], "median_ms": float(np.median(ev)), "min_ms": float(min(ev)),
                           "p90_ms": float(np.percentile(ev, 90)), "wall_median_ms": float(np.median(wall))}

    # ---- today's route to the top 1,024: xe_map_scan of everything into host memory, then numpy.argpartition
    hk, hv = np.zeros((entries, 16), np.uint8), np.zeros((entries, 16), np.uint8)
    tk, tv = np.zeros((1024, 16), np.uint8), np.zeros((1024, 16), np.uint8)
    order8 = N.MapOrder(0, 8, 1, 0)
    today, host_top = [], []
    for rep in range(3 + a.reps):
        cnt, cut = C.c_uint64(), C.c_uint64()
        t0 = time.perf_counter()
        assert lib.map_scan(vm.h, m, None, hk.ctypes.data, hv.ctypes.data, entries, C.byref(cnt)) == 0
        f = hv.view(np.uint64)[:, 0]
        idx = np.argpartition(f, entries - 1024)[entries - 1024:]
        sel_k, sel_v = hk[idx], hv[idx]
        t1 = time.perf_counter()
        assert lib.map_top(vm.h, m, None, C.byref(order8), tk.ctypes.data, tv.ctypes.data, 1024, C.byref(cnt), C.byref(cut)) == 0
        t2 = time.perf_counter()
        if rep >= 3:
            today.append((t1 - t0) * 1e3)
            host_top.append((t2 - t1) * 1e3)
    assert set(map(bytes, sel_k)) == set(map(bytes, tk)) == set(map(bytes, k_mark)) and len(sel_v) == 1024
    out["today"] = {"scan_all_to_host_then_argpartition_ms": {"what": "xe_map_scan of every entry into host memory + numpy.argpartition (wall)",
                                                              "calls": len(today), "median": float(np.median(today)), "min": float(min(today))},
                    "map_top_1024_w8_host_ms": {"what": "xe_map_top (host pointers), k = 1,024 (wall)", "calls": len(host_top),
                                                "median": float(np.median(host_top)), "min": float(min(host_top))}}
    base = out["calls"]["count_only_filtered"]["median_ms"]
    acc = {"count_only_filtered_median_ms": base}
    for width in (4, 8):
        ms = out["calls"][f"top_1024_w{width}"]["median_ms"]
        acc[f"top_1024_w{width}"] = {"median_ms": ms, "bound_ms": (width + 2) * base, "passes_allowed": width + 2,
                                     "in_count_only_scans": ms / base, "within_bound": ms <= (width + 2) * base}
    t_old, t_new = out["today"]["scan_all_to_host_then_argpartition_ms"]["median"], out["today"]["map_top_1024_w8_host_ms"]["median"]
    acc["against_today"] = {"today_ms": t_old, "map_top_ms": t_new, "today_over_map_top": t_old / t_new, "faster": t_new < t_old}
    out["acceptance"] = acc
    out["whole_map_traffic"] = dict(zip(("uploads", "downloads"), vm.map_traffic(m)))
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
