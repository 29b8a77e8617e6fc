#!/usr/bin/env python3
"""Time the device-side LRU_HASH calls (xe_lru_lookup_batch_device, xe_lru_delete_batch_device, xe_lru_order_device,
xe_lru_evict_device) on the flow table of the C3-LRU-full benchmark config (LRU_HASH, 16-byte keys and values,
1,048,576 entries, full), after a batch run has made the device copy the newer one, beside what the host calls
offer for the same answers, measured in the same run.

    python scripts/prof_maplru.py --out profiles/mapops/maplru.json

Device cases (medians of --reps single blocking calls, device events on one stream, and the wall clock beside them):
  lookup_1024          a promoting lookup of 1,024 present keys;
  peek_1024            the same keys under XE_LRU_PEEK;
  oldest_1024          the 1,024 least recently used entries, keys and values;
  delete_65536         65,536 present keys deleted;
  evict_65536          the 65,536 least recently used entries removed, keys and values reported.
There is no device-side LRU update to put entries back with, so every delete / evict call removes the NEXT 65,536
entries of a table that shrinks (its slots, which the selection walks, stay the same); two warm-up calls remove
1,024 each. The evicts run on a second VM set up the same way, the host cases on a third (the full table).

Host cases (wall clock, --host-reps each; every one ends with a one-key device peek, so a host-dirty map pays the
upload the next device call would pay):
  host_lookup_1024         xe_map_lookup x 1,024 (the first downloads the map, each promotes in the mirror);
  host_oldest_1024         xe_map_lru_order + xe_map_dump and a numpy slice and join by key of the last 1,024;
  host_delete_1024         xe_map_delete x 1,024: a SAMPLE. 65,536 one-by-one deletes cost about 64 times that
                           (each searches and shifts the mirror's list) and were not run; the JSON says so and
                           gives the per-key time, not a measured 65,536-key figure.
Before any timing the device's oldest 1,024 are compared with the tail of xe_map_lru_order."""
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

SMALL, LARGE, PEEK, OLDEST = 1024, 65536, 1, 1


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1024 * 1024, help="packets of the populating batch")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_maplru: no GPU")
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import VM, Settings

    n = a.packets
    umem, descs = W.build_batch("c3lrufull", 0, n)
    d_umem = torch.from_numpy(umem).cuda()
    d_desc = torch.from_numpy(descs.view(np.uint8)).cuda()
    d_ver = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    m = 1

    def fresh_vm() -> VM:
        vm = VM(Settings())
        W.setup_vm(vm, "c3lrufull")
        torch.cuda.synchronize()
        vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_verdicts=d_ver.data_ptr(), stream=s)
        torch.cuda.synchronize()
        return vm

    vm = fresh_vm()
    lib = vm.lib

    def ok(rc) -> None:
        assert rc == 0, (rc, lib.last_error(vm.h))

    def order(v: VM, k: int, flags: int, keys, vals, evict: bool = False) -> int:
        cnt = C.c_uint64()
        fn = lib.lru_evict_device if evict else lib.lru_order_device
        rc = fn(v.h, m, None, flags, keys.data_ptr() if keys is not None else None, vals.data_ptr() if vals is not None else None,
                k, C.byref(cnt), s)
        assert rc == 0, (rc, lib.last_error(v.h))
        return cnt.value

    entries = order(vm, 0, 0, None, None)
    all_keys = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    r_keys = torch.empty((LARGE, 16), dtype=torch.uint8, device="cuda")
    r_vals = torch.empty((LARGE, 16), dtype=torch.uint8, device="cuda")
    l_vals = torch.empty((LARGE, 16), dtype=torch.uint8, device="cuda")
    l_found = torch.empty(LARGE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert order(vm, entries, 0, all_keys, None) == entries
    traffic0 = vm.map_traffic(m)

    # ---- the answer checked once: the oldest 1,024 against the tail of xe_map_lru_order (one download)
    assert order(vm, SMALL, OLDEST, r_keys, r_vals) == entries
    host_order = vm.map_lru_order(m)
    assert len(host_order) == entries
    assert r_keys[:SMALL].cpu().numpy().tobytes() == b"".join(host_order[::-1][:SMALL]), "the device's oldest differ from the usage list's tail"
    assert all_keys.cpu().numpy().tobytes() == b"".join(host_order), "the device's order differs from xe_map_lru_order"
    del host_order

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

    def summary(v) -> dict:
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        return {"calls": len(v), "median_ms": float(np.median(ev)), "min_ms": float(min(ev)), "p90_ms": float(np.percentile(ev, 90)),
                "wall_median_ms": float(np.median(wall))}

    # ---- the calls that remove nothing, interleaved
    g = torch.Generator(device="cpu").manual_seed(1)
    perm = torch.randperm(entries, generator=g).cuda()
    look_keys = all_keys[perm[:SMALL]].contiguous()
    torch.cuda.synchronize()

    def lookup(flags: int) -> None:
        ok(lib.lru_lookup_batch_device(vm.h, m, look_keys.data_ptr(), SMALL, l_vals.data_ptr(), l_found.data_ptr(), flags, s))

    calls = {"lookup_1024": lambda: lookup(0), "peek_1024": lambda: lookup(PEEK),
             "oldest_1024": lambda: order(vm, SMALL, OLDEST, r_keys, r_vals)}
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):
        for k, fn in calls.items():
            t = timed(fn)
            if rep >= 3:
                times[k].append(t)
    assert bool(l_found[:SMALL].all()), "a present key was not found"
    res = {k: summary(v) for k, v in times.items()}

    # ---- deletes: the next 65,536 present keys each call
    del_keys = all_keys[perm[SMALL:]].contiguous()
    torch.cuda.synchronize()
    at = 0

    def delete(count: int) -> None:
        nonlocal at
        ok(lib.lru_delete_batch_device(vm.h, m, del_keys[at:at + count].data_ptr(), count, l_found.data_ptr(), s))
        at += count

    reps = min(a.reps, (len(del_keys) - 2 * SMALL) // LARGE)
    for _ in range(2):
        timed(lambda: delete(SMALL))
    dt = [timed(lambda: delete(LARGE)) for _ in range(reps)]
    assert bool(l_found.all()) and order(vm, 0, 0, None, None) == entries - at, "the deletes did not remove what they were given"
    res["delete_65536"] = summary(dt)
    assert vm.map_traffic(m)[0] == traffic0[0] and vm.map_traffic(m)[1] == traffic0[1] + 1, "a device call moved the whole map"
    vm.close()

    # ---- evicts, on a second VM set up the same way
    vm = fresh_vm()
    for _ in range(2):
        timed(lambda: order(vm, SMALL, OLDEST, r_keys, r_vals, evict=True))
    et = [timed(lambda: order(vm, LARGE, OLDEST, r_keys, r_vals, evict=True)) for _ in range(reps)]
    assert order(vm, 0, 0, None, None) == entries - 2 * SMALL - reps * LARGE
    res["evict_65536"] = summary(et)

    vm.close()

    # ---- what the host calls offer, on a third VM set up the same way: the full table (each ends with a one-key
    # device peek)
    vm = fresh_vm()
    left = order(vm, 0, 0, None, None)
    some = torch.empty((left, 16), dtype=torch.uint8, device="cuda")
    order(vm, left, 0, some, None)
    host_keys = some.cpu().numpy()[np.random.default_rng(2).permutation(left)[:2 * SMALL * a.host_reps]]

    def peek_one() -> None:
        ok(lib.lru_lookup_batch_device(vm.h, m, look_keys.data_ptr(), 1, l_vals.data_ptr(), l_found.data_ptr(), PEEK, s))

    def touch_one() -> None:  # a promoting lookup: the device copy becomes the newer one
        ok(lib.lru_lookup_batch_device(vm.h, m, look_keys.data_ptr(), 1, l_vals.data_ptr(), l_found.data_ptr(), 0, s))

    def wall(fn) -> float:
        t0 = time.perf_counter()
        fn()
        peek_one()
        return (time.perf_counter() - t0) * 1e3

    def host_lookup(keys) -> None:
        for k in keys:
            assert vm.map_lookup(m, k.tobytes()) is not None

    def host_oldest() -> None:
        usage = vm.map_lru_order(m)
        dk, dv = vm.map_dump(m)
        table = {k.tobytes(): i for i, k in enumerate(dk)}
        tail = usage[::-1][:SMALL]
        host_oldest.vals = dv[[table[k] for k in tail]]

    def host_delete(keys) -> None:
        for k in keys:
            vm.map_delete(m, k.tobytes())

    host = {"host_lookup_1024": [], "host_oldest_1024": [], "host_delete_1024": []}
    for rep in range(a.host_reps):
        touch_one()  # the device copy is the newer one again: the host call downloads
        host["host_lookup_1024"].append(wall(lambda: host_lookup(host_keys[rep * SMALL:(rep + 1) * SMALL])))
        touch_one()
        host["host_oldest_1024"].append(wall(host_oldest))
        touch_one()
        lo = (a.host_reps + rep) * SMALL
        host["host_delete_1024"].append(wall(lambda: host_delete(host_keys[lo:lo + SMALL])))
    for k, v in host.items():
        res[k] = {"calls": len(v), "wall_median_ms": float(np.median(v)), "wall_min_ms": float(min(v))}
    per_key = res["host_delete_1024"]["wall_median_ms"] / SMALL
    res["host_delete_1024"]["note"] = ("a sample of 1,024 one-by-one deletes including one download and one upload of the map; "
                                       "65,536 of them were not run")
    res["host_delete_1024"]["per_key_ms"] = per_key
    out = {"map": {"type": "LRU_HASH", "key_size": 16, "value_size": 16, "max_entries": W.C3_MAX, "entries": entries, "config": "c3lrufull"},
           "batch_packets": n, "entries_for_host_cases": left, "calls": res,
           "removing_calls": "every delete / evict call removes the next 65,536 entries; nothing is put back",
           "host_over_device": {"lookup_1024": res["host_lookup_1024"]["wall_median_ms"] / res["lookup_1024"]["wall_median_ms"],
                                "oldest_1024": res["host_oldest_1024"]["wall_median_ms"] / res["oldest_1024"]["wall_median_ms"]},
           "whole_map_traffic": dict(zip(("uploads", "downloads"), vm.map_traffic(m)))}
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
