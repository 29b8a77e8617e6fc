#!/usr/bin/env python3
"""Time the device-side join (xe_map_join_device) on C5's flow table (BASELINE configs[4]: HASH, 16-byte keys and
values, 1,048,576 entries, full), after a C5 batch has made the device copy the newer one, against a second HASH
map keyed by the 4-byte source address that holds every second source (a blocklist), beside the composition of
calls that gives the same answers without it, measured in the same run.

    python scripts/prof_mapjoin.py --out profiles/mapops/mapjoin.json

Cases (the key of C5 is {saddr, daddr, sport, dport, proto, pad}; the join key is key bytes 0 .. 3):
  count_absent / count_present   count only: an anti-join and a semi-join of every flow;
  report_1024                    the first 1,024 flows whose source is listed: keys and values;
  report_1024_other_values       the same with the blocklist's values beside them (the inner join);
  remove_65536                   the first 65,536 flows whose source is listed removed, their keys and values reported
                                 (put back outside the timed region: the records are taken again).
The composition ("composed_*"): xe_map_scan_device of every entry (keys and values), a torch slice of the join
bytes, xe_map_lookup_batch_device on the blocklist (values and found), a torch mask and compress of the first r
rows, and for the removal xe_map_delete_batch_device of the r keys. scan_count_only is xe_map_scan_device counting
every entry (SELECT and SCAN alone): what the join's fused probe adds is count_* minus it.
Before any timing every case's answer is compared with a whole-table scan joined by numpy, and the composition's
with the join's.

Calls: device events around single blocking calls on one stream, after warm-up, interleaved case by case; each
library call ends with its own stream synchronisation; medians, minima and 90th percentiles over --reps calls,
and the wall-clock median beside the events'."""
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

REPORT, REMOVE = 1024, 65536


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4 * 1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_mapjoin: no GPU")
    from gobpfld_amd import _native as N
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import MAP_HASH, MG_KEY, MJ_ABSENT, MJ_PRESENT, MJ_REMOVE, VM, MapDef, Settings

    vm = VM(Settings())
    W.setup_vm(vm, "c5")
    m = 1
    block = vm.add_map(MapDef(MAP_HASH, 4, 16, 1 << 20))
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
    d_other = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    d_found = torch.empty(entries, dtype=torch.uint8, device="cuda")
    r_keys = torch.empty((REMOVE, 16), dtype=torch.uint8, device="cuda")
    r_vals = torch.empty((REMOVE, 16), dtype=torch.uint8, device="cuda")
    r_other = torch.empty((REMOVE, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def ok(rc) -> None:
        assert rc == 0, (rc, lib.last_error(vm.h))

    def scan(cap: int) -> int:
        cnt = C.c_uint64()
        ok(lib.map_scan_device(vm.h, m, None, d_keys.data_ptr() if cap else None, d_vals.data_ptr() if cap else None, cap, C.byref(cnt), s))
        return cnt.value

    def join(mode: int, cap: int, keys=None, vals=None, other=None, flags: int = 0) -> tuple[int, int]:
        j = N.MapJoin(MG_KEY, 0, 4, mode, flags, 0)
        cnt, sel = C.c_uint64(), C.c_uint64()
        ok(lib.map_join_device(vm.h, m, None, C.byref(j), block, keys.data_ptr() if keys is not None else None,
                               vals.data_ptr() if vals is not None else None, other.data_ptr() if other is not None else None, cap,
                               C.byref(cnt), C.byref(sel), s))
        return cnt.value, sel.value

    def put_back(keys, vals, count: int) -> None:
        if count:
            ok(lib.map_update_batch_device(vm.h, m, keys.data_ptr(), vals.data_ptr(), count, s))

    # ---- the blocklist: every second source address of the table, and the answers by numpy
    assert scan(entries) == entries
    all_k, all_v = d_keys.cpu().numpy().copy(), d_vals.cpu().numpy().copy()
    saddr = np.ascontiguousarray(all_k[:, 0:4]).view(np.uint32).reshape(-1)
    sources = np.unique(saddr)
    listed = np.ascontiguousarray(sources[::2])
    lvals = np.zeros((len(listed), 16), dtype=np.uint8)
    lvals[:, 0:4] = listed.view(np.uint8).reshape(-1, 4)
    lvals[:, 8] = 1
    vm.map_update_batch_device(block, torch.from_numpy(listed.view(np.uint8).reshape(-1, 4).copy()).cuda(), torch.from_numpy(lvals).cuda())
    present = np.isin(saddr, listed)
    n_present = int(present.sum())
    traffic0 = vm.map_traffic(m), vm.map_traffic(block)
    assert join(MJ_PRESENT, 0) == (n_present, entries) and join(MJ_ABSENT, 0) == (entries - n_present, entries)
    assert join(MJ_PRESENT, REPORT, r_keys, r_vals, r_other) == (n_present, entries)
    assert np.array_equal(r_keys[:REPORT].cpu().numpy(), all_k[present][:REPORT]), "the join's keys differ from the numpy join"
    assert np.array_equal(r_vals[:REPORT].cpu().numpy(), all_v[present][:REPORT])
    assert np.array_equal(r_other[:REPORT, 0:4].cpu().numpy(), all_k[present][:REPORT, 0:4]) and (r_other[:REPORT, 8] == 1).all()
    assert join(MJ_PRESENT, REMOVE, r_keys, r_vals, None, MJ_REMOVE) == (n_present, entries)
    assert np.array_equal(r_keys.cpu().numpy(), all_k[present][:REMOVE])
    assert join(MJ_PRESENT, 0) == (n_present - REMOVE, entries - REMOVE)
    put_back(r_keys, r_vals, REMOVE)
    assert join(MJ_PRESENT, 0) == (n_present, entries)
    assert scan(entries) == entries and np.array_equal(d_keys.cpu().numpy(), all_k), "the removed flows did not take their old records"

    # ---- the composition
    def composed(mode: int, cap: int, other: bool = False, remove: bool = False) -> int:
        cnt = scan(entries)
        with torch.cuda.stream(stream):
            jk = d_keys[:cnt, 0:4].contiguous()
        stream.synchronize()
        ok(lib.map_lookup_batch_device(vm.h, block, jk.data_ptr(), cnt, d_other.data_ptr(), d_found.data_ptr(), s))
        with torch.cuda.stream(stream):
            mask = d_found[:cnt] == (1 if mode == MJ_PRESENT else 0)
            matched = int(mask.sum().item())
            r = min(matched, cap)
            if r:
                idx = mask.nonzero()[:r, 0]
                composed.keys, composed.vals = d_keys[idx], d_vals[idx]
                if other:
                    composed.other = d_other[idx]
        stream.synchronize()
        if remove and r:
            ok(lib.map_delete_batch_device(vm.h, m, composed.keys.data_ptr(), r, None, s))
        return matched

    assert composed(MJ_ABSENT, 0) == entries - n_present and composed(MJ_PRESENT, REPORT, other=True) == n_present
    assert np.array_equal(composed.keys.cpu().numpy(), all_k[present][:REPORT]) and np.array_equal(composed.other.cpu().numpy()[:, 8], np.ones(REPORT, np.uint8))
    assert composed(MJ_PRESENT, REMOVE, remove=True) == n_present and join(MJ_PRESENT, 0)[0] == n_present - REMOVE
    put_back(composed.keys, composed.vals, REMOVE)
    assert join(MJ_PRESENT, 0) == (n_present, entries)
    assert (vm.map_traffic(m), vm.map_traffic(block)) == traffic0, "a call moved a whole map"

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

    nothing = lambda: None  # noqa: E731
    calls = {
        "scan_count_only": (lambda: scan(0), nothing),
        "count_absent": (lambda: join(MJ_ABSENT, 0), nothing),
        "count_present": (lambda: join(MJ_PRESENT, 0), nothing),
        "report_1024": (lambda: join(MJ_PRESENT, REPORT, r_keys, r_vals), nothing),
        "report_1024_other_values": (lambda: join(MJ_PRESENT, REPORT, r_keys, r_vals, r_other), nothing),
        "remove_65536": (lambda: join(MJ_PRESENT, REMOVE, r_keys, r_vals, None, MJ_REMOVE), lambda: put_back(r_keys, r_vals, REMOVE)),
        "composed_count_absent": (lambda: composed(MJ_ABSENT, 0), nothing),
        "composed_count_present": (lambda: composed(MJ_PRESENT, 0), nothing),
        "composed_report_1024": (lambda: composed(MJ_PRESENT, REPORT), nothing),
        "composed_report_1024_other_values": (lambda: composed(MJ_PRESENT, REPORT, other=True), nothing),
        "composed_remove_65536": (lambda: composed(MJ_PRESENT, REMOVE, remove=True), lambda: put_back(composed.keys, composed.vals, REMOVE)),
    }
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):
        for k, (fn, restore) in calls.items():
            t = timed(fn)
            restore()  # outside the timed region
            if rep >= 3:
                times[k].append(t)
    res = {}
    for k, v in times.items():
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        res[k] = {"calls": len(v), "median_ms": float(np.median(ev)), "min_ms": float(min(ev)), "p90_ms": float(np.percentile(ev, 90)),
                  "wall_median_ms": float(np.median(wall))}
    assert join(MJ_PRESENT, 0) == (n_present, entries)
    med = {k: v["median_ms"] for k, v in res.items()}
    out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": entries, "slots": 2 * W.C5_MAX},
           "other": {"type": "HASH", "key_size": 4, "value_size": 16, "entries": int(len(listed)), "join": "key bytes 0..3"},
           "batch_packets": n, "sources": int(len(sources)), "present": n_present, "calls": res,
           "composed_over_join": {k: med["composed_" + k] / med[k] for k in med if "composed_" + k in med},
           "join_minus_scan_count_only_ms": {k: med[k] - med["scan_count_only"] for k in ("count_absent", "count_present")},
           "whole_map_traffic": dict(zip(("uploads", "downloads"), vm.map_traffic(m)))}
    # SELECT and SCAN over the same table as the commit before the join recorded them (a count-only call of
    # scripts/prof_mapmodify.py): scan_count_only above is the same, unchanged code measured in this run
    before = ROOT / "profiles" / "mapops" / "mapmodify.json"
    if before.exists():
        c = json.loads(before.read_text()).get("calls", {}).get("count_only_all")
        if c:
            out["scan_count_only_parent_commit"] = {"from": "profiles/mapops/mapmodify.json count_only_all",
                                                    **{k: c[k] for k in ("median_ms", "min_ms", "p90_ms")}}
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
