#!/usr/bin/env python3
"""Time the batched device map calls (xe_map_lookup_batch_device / _update_ / _delete_) on C5's flow
table (BASELINE configs[4]: HASH, 16-byte keys and values, 1,048,576 entries, full), after one C5 batch
has made the device copy the newer one, beside what a caller of the single-key calls pays for the same
access: the download of the whole map, and its upload before the next batch.

    python scripts/prof_mapops.py --out profiles/mapops/mapops.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/prof_mapops.py --trace-run   # kernel times

Before anything is timed, a 4,096-key sample of every call's output is compared for equality with the
single-key path (xe_map_lookup after the call).

Baseline (wall clock around the blocking calls, the batches with their stream synchronised):
  download   one xe_map_lookup while the device copy is newer
  reupload   one xe_map_update, then the next batch's time over a clean batch's
New calls: device events around single calls on one stream, after warm-up; each call ends with its own
stream synchronisation, so the event time is what the caller waits for. The 65,536-key delete and the
65,536-key insert of absent keys alternate (the table is full: the insert needs the room the delete made;
C5's last 65,536 keys make room for as many new ones, then those for C5's again).

Algorithmic bytes of a lookup, per key: one 64-byte group of slot records, one 16-byte value, 16 bytes of
key in, 16 of value out, 1 of found. Shares are of the 6.3 TB/s achievable HBM rate.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_TBS = 6.3
LOOKUP_BYTES = {"record_group": 64, "value": 16, "key_in": 16, "value_out": 16, "found": 1}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4 * 1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-run", action="store_true", help="a short run for a kernel trace: 5 calls each, no baseline")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_mapops: no GPU")
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import VM, Settings

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

    def batch() -> float:  # wall ms of one synchronous batch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_verdicts=d_ver.data_ptr(), stream=s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):
        batch()  # (the first compiles the kernel and uploads the table)

    keys, _ = W.c5_map_entries()
    rng = np.random.default_rng(5)
    present = np.ascontiguousarray(keys[rng.permutation(len(keys))])
    absent = np.ascontiguousarray(W.key_from_tuple(W.flow_tuples(5, np.arange(1 << 20, dtype=np.uint64) + np.uint64(1 << 30))))
    assert not (set(map(bytes, absent[:4096])) & set(map(bytes, keys[:4096])))
    d_present, d_absent = torch.from_numpy(present).cuda(), torch.from_numpy(absent).cuda()
    big = 1 << 20
    d_vals = torch.empty((big, 16), dtype=torch.uint8, device="cuda")
    d_found = torch.empty(big, dtype=torch.uint8, device="cuda")
    new_vals = torch.from_numpy(rng.integers(0, 256, size=(big, 16), dtype=np.uint8)).cuda()

    def lookup(d_k, cnt):
        rc = lib.map_lookup_batch_device(vm.h, m, d_k.data_ptr(), cnt, d_vals.data_ptr(), d_found.data_ptr(), s)
        assert rc == 0, rc

    def update(d_k, cnt, d_v=new_vals):
        rc = lib.map_update_batch_device(vm.h, m, d_k.data_ptr(), d_v.data_ptr(), cnt, s)
        assert rc == 0, (rc, lib.last_error(vm.h))

    def delete(d_k, cnt):
        rc = lib.map_delete_batch_device(vm.h, m, d_k.data_ptr(), cnt, d_found.data_ptr(), s)
        assert rc == 0, rc

    # ---- equality with the single-key path on a 4,096-key sample of every call, before any timing
    S = 4096
    traffic0 = vm.map_traffic(m)
    lookup(d_present, S)
    got_v, got_f = d_vals[:S].cpu().numpy(), d_found[:S].cpu().numpy()
    lookup(d_absent, S)
    abs_v, abs_f = d_vals[:S].cpu().numpy(), d_found[:S].cpu().numpy()
    update(d_present[S:], S)
    delete(d_present[2 * S:], S)
    del_f = d_found[:S].cpu().numpy()
    update(d_absent, S // 2)  # (room: 4,096 were deleted)
    assert vm.map_traffic(m) == traffic0, "a batched device call moved the whole map"
    nv = new_vals[:S].cpu().numpy()
    for i in range(S):  # (the first single-key call downloads the map)
        assert vm.map_lookup(m, present[2 * S + i].tobytes()) is None
        assert vm.map_lookup(m, present[S + i].tobytes()) == nv[i].tobytes()
        one = vm.map_lookup(m, present[i].tobytes())
        assert got_f[i] == 1 and one == got_v[i].tobytes()
        assert vm.map_lookup(m, absent[i].tobytes()) == (nv[i].tobytes() if i < S // 2 else None)
    assert not abs_f.any() and not abs_v.any() and del_f.all()
    delete(d_absent, S // 2)  # back to C5's key set
    update(d_present[2 * S:], S)
    assert vm.map_count(m) == len(keys)

    out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": len(keys)},
           "batch_packets": n, "hbm_achievable_tbs": HBM_TBS, "verified_sample": S, "baseline": {}, "calls": {}}

    # ---- the baseline: what one key costs through the host mirror
    if not a.trace_run:
        down, reup, clean, one_key = [], [], [], []
        for _ in range(3):
            clean.append(batch())  # the device copy is the newer one again
            t0 = time.perf_counter()
            vm.map_lookup(m, present[0].tobytes())
            down.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            vm.map_update(m, present[0].tobytes(), bytes(16))
            one_key.append((time.perf_counter() - t0) * 1e3)
            reup.append(batch())
            clean.append(batch())
        base_clean = float(np.median(clean))
        out["baseline"] = {
            "download_ms": {"what": "one xe_map_lookup while the device copy is newer (wall)", "runs": down, "median": float(np.median(down))},
            "reupload_ms": {"what": "the batch after one xe_map_update, over a clean batch (wall)", "runs": [r - base_clean for r in reup],
                            "median": float(np.median(reup)) - base_clean},
            "clean_batch_ms": base_clean, "host_update_ms": float(np.median(one_key))}
        batch()

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    K = 65536
    d_new = d_absent[K:]  # absent keys the sample did not touch
    calls = {}
    for cnt in (1, 1024, big):
        calls[f"lookup_present_{cnt}"] = lambda cnt=cnt: lookup(d_present, cnt)
        calls[f"lookup_absent_{cnt}"] = lambda cnt=cnt: lookup(d_absent, cnt)
    calls["update_present_1024"] = lambda: update(d_present, 1024)
    calls[f"update_present_{big}"] = lambda: update(d_present, big)
    d_tail = d_present[big - K:]

    def churn(t_del: list, t_ins: list) -> None:  # one cycle: C5's last 65,536 keys out, new ones in, and back
        for out_keys, in_keys in ((d_tail, d_new), (d_new, d_tail)):
            t_del.append(timed(lambda: delete(out_keys, K)))
            t_ins.append(timed(lambda: update(in_keys, K)))

    reps = 5 if a.trace_run else a.reps
    times = {k: [] for k in calls}
    times[f"delete_{K}"], times[f"update_new_{K}"] = [], []
    for k, fn in calls.items():
        for _ in range(3):
            timed(fn)
    churn([], [])
    for _ in range(reps):  # the variants take turns
        for k, fn in calls.items():
            times[k].append(timed(fn))
        churn(times[f"delete_{K}"], times[f"update_new_{K}"])
    assert vm.map_count(m) == len(keys)
    torch.cuda.synchronize()
    if a.trace_run:
        print("trace run done:", {k: len(v) for k, v in times.items()})
        vm.close()
        return
    for k, v in times.items():
        row = {"calls": len(v), "median_ms": float(np.median(v)), "min_ms": float(min(v)), "p90_ms": float(np.percentile(v, 90))}
        cnt = int(k.rsplit("_", 1)[1])
        row["keys"] = cnt
        row["keys_per_s"] = cnt / (row["median_ms"] * 1e-3)
        if k.startswith("lookup") and cnt == big:
            per = sum(LOOKUP_BYTES.values())
            tbs = cnt * per / (row["median_ms"] * 1e-3) / 1e12
            row.update({"algorithmic_bytes_per_key": LOOKUP_BYTES, "achieved_tbs": tbs, "share_of_hbm": tbs / HBM_TBS})
        out["calls"][k] = row
    b = out["baseline"]
    acc = {}
    for k in ("lookup_present_1024", "update_present_1024"):
        ms = out["calls"][k]["median_ms"]
        acc[k] = {"median_ms": ms, "download_over_call": b["download_ms"]["median"] / ms, "reupload_over_call": b["reupload_ms"]["median"] / ms,
                  "cheaper_than_download": ms < b["download_ms"]["median"], "cheaper_than_reupload": ms < b["reupload_ms"]["median"]}
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
