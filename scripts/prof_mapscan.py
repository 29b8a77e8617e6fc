#!/usr/bin/env python3
"""Time the device-side map scan and expire (xe_map_scan_device / xe_map_expire_device) on C5's flow table
(BASELINE configs[4]: HASH, 16-byte keys and values, 1,048,576 entries, full), after a C5 batch has made
the device copy the newer one, beside what they replace, measured in the same run: xe_map_dump while the
device copy is newer, which downloads the whole map before the caller can filter anything.

    python scripts/prof_mapscan.py --out profiles/mapops/mapscan.json

The values of C5 are {packets, bytes} counters. Before anything is timed, 1,024 entries get bit 41 of the
packet count set and 65,536 others bit 40 (xe_map_update_batch_device; the batches only add to the low
bits), so `ANYBITS 1 << 41` at offset 0 selects exactly the former and `ANYBITS 1 << 40` the latter. What
the calls report is compared with the keys installed and, for a sample, with the single-key path.

Calls: device events around single calls on one stream, after warm-up, the variants taking turns; each
call ends with its own stream synchronisation, so the event time is what the caller waits for. The expire
removes 65,536 entries each time; they are installed again outside the timed region.

Algorithmic bytes of the whole-table scan: the slot records (word 0 of every record: every 64-byte group
of the record array is touched), the 64-byte lines that hold the FULL records' fields, the bitmap (written
by SELECT, read by SCATTER) and the outputs (keys and values of every entry). Shares are of the 6.3 TB/s
achievable HBM rate that profiles/mapops/mapops.json uses.
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

HBM_TBS = 6.3
MARK_EXPIRE, MARK_SCAN = 1 << 40, 1 << 41
N_SCAN, N_EXPIRE = 1024, 65536


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4 * 1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_mapscan: no GPU")
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
    rng = np.random.default_rng(6)
    order = rng.permutation(entries)
    k_scan = np.ascontiguousarray(keys[order[:N_SCAN]])
    k_exp = np.ascontiguousarray(keys[order[N_SCAN:N_SCAN + N_EXPIRE]])

    def marked(cnt: int, mark: int) -> np.ndarray:
        v = np.zeros((cnt, 2), dtype=np.uint64)
        v[:, 0] = np.uint64(mark) + np.arange(cnt, dtype=np.uint64) * np.uint64(mark == MARK_SCAN)
        v[:, 1] = 64
        return v.view(np.uint8).reshape(cnt, 16)

    d_kscan, d_vscan = torch.from_numpy(k_scan).cuda(), torch.from_numpy(marked(N_SCAN, MARK_SCAN)).cuda()
    d_kexp, d_vexp = torch.from_numpy(k_exp).cuda(), torch.from_numpy(marked(N_EXPIRE, MARK_EXPIRE)).cuda()
    d_keys = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_vals = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def install(d_k, d_v) -> None:
        rc = lib.map_update_batch_device(vm.h, m, d_k.data_ptr(), d_v.data_ptr(), len(d_k), s)
        assert rc == 0, (rc, lib.last_error(vm.h))

    f_all = N.MapFilter(MF_ALL, 0, 0, 0, 0)
    f_scan = N.MapFilter(MF_ANYBITS, 0, 8, 0, MARK_SCAN)
    f_exp = N.MapFilter(MF_ANYBITS, 0, 8, 0, MARK_EXPIRE)

    def scan(flt, cap: int, out: bool = True, expire: bool = False) -> int:
        cnt = C.c_uint64()
        fn = lib.map_expire_device if expire else lib.map_scan_device
        rc = fn(vm.h, m, C.byref(flt), d_keys.data_ptr() if out else None, d_vals.data_ptr() if out else None, cap, C.byref(cnt), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value

    install(d_kscan, d_vscan)
    install(d_kexp, d_vexp)
    traffic0 = vm.map_traffic(m)

    # ---- what the calls report, before any timing
    def as_set(t) -> set:
        return set(map(bytes, t.cpu().numpy()))

    assert scan(f_all, 0, out=False) == entries
    assert scan(f_scan, entries) == N_SCAN and as_set(d_keys[:N_SCAN]) == set(map(bytes, k_scan))
    assert np.array_equal(np.sort(d_vals[:N_SCAN].cpu().numpy().view(np.uint64)[:, 0]), np.uint64(MARK_SCAN) + np.arange(N_SCAN, dtype=np.uint64))
    assert scan(f_exp, entries) == N_EXPIRE and as_set(d_keys[:N_EXPIRE]) == set(map(bytes, k_exp))
    assert scan(f_all, entries) == entries
    all_k, all_v = d_keys.cpu().numpy(), d_vals.cpu().numpy()
    assert len(set(map(bytes, all_k))) == entries
    assert scan(f_exp, entries, expire=True) == N_EXPIRE and as_set(d_keys[:N_EXPIRE]) == set(map(bytes, k_exp))
    assert scan(f_exp, 0, out=False) == 0 and scan(f_all, 0, out=False) == entries - N_EXPIRE
    assert vm.map_traffic(m) == traffic0, "a scan or an expire moved the whole map"
    S = 4096
    expired = set(map(bytes, k_exp))
    for i in range(S):  # the single-key path (its first call downloads the map)
        one = vm.map_lookup(m, all_k[i].tobytes())
        assert one == (None if all_k[i].tobytes() in expired else all_v[i].tobytes())
    install(d_kexp, d_vexp)
    assert vm.map_count(m) == entries

    out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": entries, "slots": 2 * W.C5_MAX},
           "batch_packets": n, "hbm_achievable_tbs": HBM_TBS, "verified_sample": S, "baseline": {}, "calls": {}}

    # ---- the baseline: xe_map_dump while the device copy is the newer one
    down, full = [], []
    hk, hv = np.zeros((entries, 16), np.uint8), np.zeros((entries, 16), np.uint8)
    for _ in range(5):
        batch()
        cnt = C.c_uint64()
        t0 = time.perf_counter()
        assert lib.map_dump(vm.h, m, None, None, 0, C.byref(cnt)) == 0  # the size query: the download happens here
        t1 = time.perf_counter()
        assert lib.map_dump(vm.h, m, hk.ctypes.data, hv.ctypes.data, cnt.value, C.byref(cnt)) == 0
        t2 = time.perf_counter()
        down.append((t1 - t0) * 1e3)
        full.append((t2 - t0) * 1e3)
    out["baseline"] = {"dump_download_ms": {"what": "xe_map_dump's size query while the device copy is newer: the download (wall)",
                                            "runs": down, "median": float(np.median(down))},
                       "dump_total_ms": {"what": "... and the copy of every entry to the caller (wall)", "runs": full,
                                         "median": float(np.median(full))}}
    batch()

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

    def expire_once() -> None:
        assert scan(f_exp, N_EXPIRE, expire=True) == N_EXPIRE

    calls = {
        "count_only_all": (lambda: scan(f_all, 0, out=False), entries),
        "count_only_filtered": (lambda: scan(f_scan, 0, out=False), N_SCAN),
        f"scan_{N_SCAN}": (lambda: scan(f_scan, entries), N_SCAN),
        "scan_all": (lambda: scan(f_all, entries), entries),
        f"expire_{N_EXPIRE}": (expire_once, N_EXPIRE),
    }
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):  # three rounds of warm-up, then the variants take turns
        for k, (fn, _) in calls.items():
            t = timed(fn)
            if k.startswith("expire"):
                install(d_kexp, d_vexp)  # outside the timed region
            if rep >= 3:
                times[k].append(t)
    assert vm.map_count(m) == entries
    for k, v in times.items():
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        row = {"calls": len(v), "selected": calls[k][1], "median_ms": float(np.median(ev)), "min_ms": float(min(ev)),
               "p90_ms": float(np.percentile(ev, 90)), "wall_median_ms": float(np.median(wall))}
        if k == "scan_all":
            slots = 2 * W.C5_MAX
            parts = {"records": slots * 32, "field_lines": min(entries * 64, slots * 16), "bitmap": 2 * (slots // 8),
                     "outputs": entries * 32}
            tbs = sum(parts.values()) / (row["median_ms"] * 1e-3) / 1e12
            row.update({"algorithmic_bytes": parts, "algorithmic_bytes_total": sum(parts.values()), "achieved_tbs": tbs,
                        "share_of_hbm": tbs / HBM_TBS})
        out["calls"][k] = row
    ms, dl = out["calls"][f"scan_{N_SCAN}"]["median_ms"], out["baseline"]["dump_download_ms"]["median"]
    out["acceptance"] = {f"scan_{N_SCAN}": {"median_ms": ms, "download_ms": dl, "download_over_scan": dl / ms,
                                            "cheaper_than_download": ms < dl}}
    out["whole_map_traffic"] = dict(zip(("uploads", "downloads"), vm.map_traffic(m)))
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
