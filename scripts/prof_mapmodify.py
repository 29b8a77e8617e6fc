#!/usr/bin/env python3
"""Time the device-side in-place edit of map value fields (xe_map_modify_device / xe_map_modify_batch_device)
on C5's flow table (BASELINE configs[4]: HASH, 16-byte keys and values, 1,048,576 entries, 2^21 slots, full),
after a C5 batch has made the device copy the newer one, beside the two ways a caller had before, measured in
the same run:

  * the device round trip, made of existing calls only: xe_map_scan_device of the selected entries into device
    buffers, a torch kernel that edits the values, xe_map_update_batch_device, which probes the table again
    for every key it has just read;
  * the host path: xe_map_dump (the download), a numpy edit, xe_map_update_batch, and the upload that the next
    device call makes.

    python scripts/prof_mapmodify.py --out profiles/mapops/mapmodify.json

The values of C5 are {packets, bytes} counters. Before anything is timed 65,536 entries get bit 40 of the
packet count set (xe_map_update_batch_device; the batches only add to the low bits), so `ANYBITS 1 << 40` at
offset 0 selects exactly those. The timed edits can be repeated without harm and leave the marks alone: the
walks SET the bytes counter (offset 8) to 0, which is the read-and-reset job; the token bucket treats the
bytes counter as {tokens u32, rate u32}: tokens = min(tokens +sat rate, 2^20) with the rate read from the
value, then rate |= 1 (three edits, one with XE_MM_OPERAND_FIELD; repeated, the tokens stop at the cap). What
the calls leave is compared with the single-key path for a sample before the timing starts.

Calls: device events around single calls on one stream, after warm-up, the variants taking turns; each call
ends with its own stream synchronisation, so the event time is what the caller waits for.

The floor of the silent walk: one read of word 0 of every record (every 64-byte group of the record array is
touched: 32 bytes a slot) plus a read and two writes (the map and the delta base) of the selected values.
Shares are of the 6.3 TB/s achievable HBM rate that profiles/mapops/mapops.json uses.
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
MARK = 1 << 40
N_MARK = 65536


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4 * 1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_mapmodify: no GPU")
    from gobpfld_amd import _native as N
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import (MF_ALL, MF_ANYBITS, MM_ADD_SAT, MM_MIN, MM_OPERAND_FIELD, MM_OR, MM_SET, VM, Settings)

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
    slots = 2 * W.C5_MAX
    rng = np.random.default_rng(7)
    k_mark = np.ascontiguousarray(keys[rng.permutation(entries)[:N_MARK]])
    v_mark = np.zeros((N_MARK, 2), dtype=np.uint64)
    v_mark[:, 0], v_mark[:, 1] = MARK, 64
    d_kmark, d_vmark = torch.from_numpy(k_mark).cuda(), torch.from_numpy(v_mark.view(np.uint8).reshape(N_MARK, 16)).cuda()
    d_keys = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_vals = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_found = torch.empty(N_MARK, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.map_update_batch_device(vm.h, m, d_kmark.data_ptr(), d_vmark.data_ptr(), N_MARK, s)
    assert rc == 0, (rc, lib.last_error(vm.h))

    f_all = N.MapFilter(MF_ALL, 0, 0, 0, 0)
    f_mark = N.MapFilter(MF_ANYBITS, 0, 8, 0, MARK)

    def edits(*e):
        arr = (N.MapEdit * len(e))(*[N.MapEdit(*x) for x in e])
        return arr, len(e)

    e_zero = edits((MM_SET, 8, 8, 0, 0))
    e_bucket = edits((MM_ADD_SAT, 8, 4, MM_OPERAND_FIELD, 12), (MM_MIN, 8, 4, 0, 1 << 20), (MM_OR, 12, 4, 0, 1))

    def modify(flt, ed, cap: int, out: bool) -> int:
        cnt = C.c_uint64()
        rc = lib.map_modify_device(vm.h, m, C.byref(flt), ed[0], ed[1], d_keys.data_ptr() if out else None,
                                   d_vals.data_ptr() if out else None, cap, C.byref(cnt), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value

    def keyed(ed, out: bool) -> None:
        rc = lib.map_modify_batch_device(vm.h, m, d_kmark.data_ptr(), N_MARK, ed[0], ed[1], d_vals.data_ptr() if out else None,
                                         d_found.data_ptr() if out else None, s)
        assert rc == 0, (rc, lib.last_error(vm.h))

    def scan(flt, cap: int) -> int:
        cnt = C.c_uint64()
        rc = lib.map_scan_device(vm.h, m, C.byref(flt), d_keys.data_ptr(), d_vals.data_ptr(), cap, C.byref(cnt), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return cnt.value

    def round_trip(flt, want: int) -> None:
        """scan -> a torch edit -> update: what a caller could do on the device before."""
        got = scan(flt, entries)
        assert got == want
        with torch.cuda.stream(stream):
            d_vals[:got, 8:16] = 0
        stream.synchronize()
        rc = lib.map_update_batch_device(vm.h, m, d_keys.data_ptr(), d_vals.data_ptr(), got, s)
        assert rc == 0, (rc, lib.last_error(vm.h))

    # ---- what the calls leave, before any timing
    traffic0 = vm.map_traffic(m)
    MAXU = (1 << 64) - 1
    assert modify(f_mark, e_zero, MAXU, out=False) == N_MARK       # the single pass
    assert modify(f_mark, e_zero, N_MARK, out=True) == N_MARK      # the general walk, reporting
    rep_k, rep_v = d_keys[:N_MARK].cpu().numpy(), d_vals[:N_MARK].cpu().numpy().view(np.uint64)
    assert set(map(bytes, rep_k)) == set(map(bytes, k_mark)) and (rep_v[:, 0] & np.uint64(MARK)).all() and not rep_v[:, 1].any()
    keyed(e_bucket, out=True)
    assert d_found.cpu().numpy().all()
    assert vm.map_traffic(m) == traffic0, "a modify moved the whole map"
    marked = set(map(bytes, k_mark))
    S, seen_marked = 4096, 0
    for i in range(S):  # the single-key path (its first call downloads the map)
        k = keys[(i * 257) % entries].tobytes()
        v = np.frombuffer(vm.map_lookup(m, k), dtype=np.uint64)
        if k in marked:  # zeroed twice, then one round of the bucket on {tokens 0, rate 0}: tokens 0, rate 1
            seen_marked += 1
            assert v[0] & np.uint64(MARK) and v[1] == np.uint64(1 << 32), v
        else:
            assert not (v[0] & np.uint64(MARK)) and v[1] % 64 == 0, v  # its bytes counter (64-byte packets) was left alone
    assert seen_marked > 100

    out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": entries, "slots": slots},
           "batch_packets": n, "hbm_achievable_tbs": HBM_TBS, "verified_sample": S, "selected": N_MARK,
           "timed_edits": "SET of the 8-byte bytes counter to 0 (repeatable); the token bucket saturates at its cap when repeated",
           "baseline_host": {}, "calls": {}}

    # ---- the host path: dump, numpy edit, update, and the next device call's upload
    hk, hv = np.zeros((entries, 16), np.uint8), np.zeros((entries, 16), np.uint8)
    parts = {"download": [], "dump_copy": [], "edit": [], "update": [], "upload": [], "total": []}
    for _ in range(3):
        batch()
        cnt = C.c_uint64()
        t0 = time.perf_counter()
        assert lib.map_dump(vm.h, m, None, None, 0, C.byref(cnt)) == 0  # the size query: the download happens here
        t1 = time.perf_counter()
        assert lib.map_dump(vm.h, m, hk.ctypes.data, hv.ctypes.data, cnt.value, C.byref(cnt)) == 0
        t2 = time.perf_counter()
        sel = (hv.view(np.uint64)[:, 0] & np.uint64(MARK)) != 0
        ek, ev = np.ascontiguousarray(hk[sel]), np.ascontiguousarray(hv[sel])
        ev[:, 8:16] = 0
        t3 = time.perf_counter()
        assert int(sel.sum()) == N_MARK
        assert lib.map_update_batch(vm.h, m, ek.ctypes.data, ev.ctypes.data, len(ek)) == 0
        t4 = time.perf_counter()
        got = C.c_uint64()
        assert lib.map_scan_device(vm.h, m, C.byref(f_mark), None, None, 0, C.byref(got), s) == 0  # uploads the map first
        t5 = time.perf_counter()
        assert got.value == N_MARK
        for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t5 - t0)):
            parts[name].append(dt * 1e3)
    out["baseline_host"] = {"what": "xe_map_dump while the device copy is newer, a numpy edit of the 65,536 selected values, "
                                    "xe_map_update_batch, a count-only device scan that uploads the map (wall ms)",
                            **{k: {"runs": v, "median": float(np.median(v))} for k, v in parts.items()}}
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

    calls = {
        "silent_zero_all": (lambda: modify(f_all, e_zero, MAXU, out=False), entries),
        f"silent_zero_{N_MARK}": (lambda: modify(f_mark, e_zero, MAXU, out=False), N_MARK),
        f"report_zero_{N_MARK}": (lambda: modify(f_mark, e_zero, N_MARK, out=True), N_MARK),
        "token_bucket_all": (lambda: modify(f_all, e_bucket, MAXU, out=False), entries),
        f"token_bucket_{N_MARK}": (lambda: modify(f_mark, e_bucket, MAXU, out=False), N_MARK),
        f"keyed_zero_{N_MARK}": (lambda: keyed(e_zero, out=False), N_MARK),
        f"keyed_zero_{N_MARK}_old_values": (lambda: keyed(e_zero, out=True), N_MARK),
        f"round_trip_{N_MARK}": (lambda: round_trip(f_mark, N_MARK), N_MARK),
        "round_trip_all": (lambda: round_trip(f_all, entries), entries),
        "count_only_all": (lambda: modify(f_all, e_zero, 0, out=False), entries),
    }
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):  # three rounds of warm-up, then the variants take turns
        for k, (fn, _) in calls.items():
            t = timed(fn)
            if rep >= 3:
                times[k].append(t)
    assert vm.map_count(m) == entries
    for k, v in times.items():
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        row = {"calls": len(v), "selected": calls[k][1], "median_ms": float(np.median(ev)), "min_ms": float(min(ev)),
               "p90_ms": float(np.percentile(ev, 90)), "wall_median_ms": float(np.median(wall))}
        if k.startswith(("silent", "token")):
            floor = {"records": slots * 32, "selected_values_read": calls[k][1] * 16, "selected_values_written_twice": calls[k][1] * 32}
            tbs = sum(floor.values()) / (row["median_ms"] * 1e-3) / 1e12
            row.update({"floor_bytes": floor, "floor_bytes_total": sum(floor.values()), "achieved_tbs": tbs, "share_of_hbm": tbs / HBM_TBS})
        out["calls"][k] = row
    c = out["calls"]
    out["comparison"] = {
        f"selected_{N_MARK}": {"single_pass_ms": c[f"silent_zero_{N_MARK}"]["median_ms"], "reporting_walk_ms": c[f"report_zero_{N_MARK}"]["median_ms"],
                               "keyed_ms": c[f"keyed_zero_{N_MARK}"]["median_ms"], "round_trip_ms": c[f"round_trip_{N_MARK}"]["median_ms"],
                               "host_path_ms": out["baseline_host"]["total"]["median"],
                               "round_trip_over_single_pass": c[f"round_trip_{N_MARK}"]["median_ms"] / c[f"silent_zero_{N_MARK}"]["median_ms"],
                               "host_path_over_single_pass": out["baseline_host"]["total"]["median"] / c[f"silent_zero_{N_MARK}"]["median_ms"]},
        "all_entries": {"single_pass_ms": c["silent_zero_all"]["median_ms"], "round_trip_ms": c["round_trip_all"]["median_ms"],
                        "round_trip_over_single_pass": c["round_trip_all"]["median_ms"] / c["silent_zero_all"]["median_ms"],
                        "single_pass_faster": c["silent_zero_all"]["median_ms"] < c["round_trip_all"]["median_ms"]},
    }
    out["whole_map_traffic"] = dict(zip(("uploads", "downloads"), vm.map_traffic(m)))
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
