#!/usr/bin/env python3
"""Time the device-side tombstone compaction (xe_map_compact) on C5's flow table (BASELINE configs[4]: HASH,
16-byte keys and values, 1,048,576 entries in 2^21 slots), after a C5 batch has made the device copy the newer
one, beside today's route to a table without tombstones, measured in the same run.

    python scripts/prof_mapcompact.py --out profiles/mapops/mapcompact.json

Tables: every 16th entry of the table in slot order (65,536) and every 2nd (524,288) removed on the device
(xe_map_delete_batch_device of their keys: the plain tombstones with key words that xe_map_expire_device leaves;
a filter on the value cannot pick flows spread over the table). Each table is kept as an exported image and put
back with xe_map_state_import outside the timed regions. Before any timing the image xe_map_compact leaves on
both is compared, byte for byte with the info, with the Python restatement of the call's definition
(tests/mapcompact_cases.py expect_compact).

Recorded, device events around single calls on one stream after warm-up, and wall clock:
  * xe_map_compact on both tables, and an XE_MC_COUNT_ONLY call;
  * today's route to the same table: a host visit (xe_map_count: download, rebuild of the mirror) plus the
    re-upload by the next device call, wall clock;
  * a 65,536-key xe_map_lookup_batch_device, half of the keys absent, and one C5 batch, on the table with
    524,288 tombstones and again after its compaction;
  * a table of 16,384 slots made of one run of kMcMaxRun slots whose entries all move up by one.

One condition is recorded under "acceptance": xe_map_compact after the removal of 65,536 entries must take less
wall-clock time than today's route.

The kernels' rows of profiles/mapops/kernel_stats.csv come from a run of this script of their own under
`rocprofv3 --kernel-trace --stats` (the xe_mapcompact_* lines of its kernel statistics, appended)."""
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
sys.path.insert(0, str(ROOT / "tests"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1024 * 1024, help="packets of the C5 batches")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-model", action="store_true", help="skip the comparison with the Python model (a profiler's run)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_mapcompact: no GPU")
    import mapcompact_cases as CC
    from gobpfld_amd import _native as N
    from gobpfld_amd import workloads as W
    from gobpfld_amd.emulator import MAP_HASH, VM, MapDef, Settings

    vm = VM(Settings())
    W.setup_vm(vm, "c5")
    m, lib = 1, vm.lib
    small = vm.add_map(MapDef(MAP_HASH, 8, 8, CC.LONG_MAX))  # the table of one long run
    n = a.packets
    umem, descs = W.build_batch("c5", 0, n)
    d_umem = torch.from_numpy(umem).cuda()
    d_desc = torch.from_numpy(descs.view(np.uint8)).cuda()
    d_ver = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def batch() -> None:
        vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_verdicts=d_ver.data_ptr(), stream=s)

    for _ in range(2):  # (the first loads or compiles the kernel and uploads the table)
        torch.cuda.synchronize()
        batch()
        torch.cuda.synchronize()
    entries = len(W.c5_map_entries()[0])
    d_keys = torch.empty((entries, 16), dtype=torch.uint8, device="cuda")
    cnt = C.c_uint64()
    torch.cuda.synchronize()
    assert lib.map_scan_device(vm.h, m, None, d_keys.data_ptr(), None, entries, C.byref(cnt), s) == 0 and cnt.value == entries
    nbytes = vm.map_state_bytes(m)

    def export() -> "torch.Tensor":
        img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.map_state_export(vm.h, m, img.data_ptr(), s) == 0
        return img

    def restore(img) -> None:
        assert lib.map_state_import(vm.h, m, img.data_ptr(), s) == 0

    def compact(flags: int = 0):
        info = N.MapCompactInfo()
        rc = lib.map_compact(vm.h, m, flags, C.byref(info), s)
        assert rc == 0, (rc, lib.last_error(vm.h))
        return info.tombstones, info.moved, info.longest_run, info.via_host

    def remove(keys) -> None:
        assert lib.map_delete_batch_device(vm.h, m, keys.data_ptr(), len(keys), None, s) == 0, lib.last_error(vm.h)

    clean = export()
    tables = {}
    for name, step in (("tombstones_65536", 16), ("tombstones_524288", 2)):
        gone = d_keys[::step].contiguous()
        torch.cuda.synchronize()
        remove(gone)
        tables[name] = export()
        restore(clean)
    traffic0 = vm.map_traffic(m)

    # ---- the answers, before any timing: against the Python model of the exported image
    infos = {}
    for name, img in tables.items():
        restore(img)
        if a.no_model:
            infos[name] = compact()
            continue
        exp = CC.expect_compact(vm, m, img.cpu().numpy(), with_host=False)
        counted = compact(CC.COUNT_ONLY)
        assert counted == (exp["info"][0], 0, exp["info"][2], 0), (counted, exp["info"])
        infos[name] = compact()
        assert infos[name] == exp["info"] and exp["info"][3] == 0, (infos[name], exp["info"])
        assert np.array_equal(export().cpu().numpy(), exp["image"]), f"{name}: the compacted image differs from the model"
    assert vm.map_traffic(m) == traffic0, "a compaction moved the whole map"

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

    def stats(v) -> dict:
        ev, wall = [t[0] for t in v], [t[1] for t in v]
        return {"calls": len(v), "median_ms": float(np.median(ev)), "min_ms": float(min(ev)), "p90_ms": float(np.percentile(ev, 90)),
                "wall_median_ms": float(np.median(wall))}

    def series(fn, before) -> dict:
        out = []
        for rep in range(3 + a.reps):
            before()  # outside the timed region
            t = timed(fn)
            if rep >= 3:
                out.append(t)
        return stats(out)

    # 65,536 keys, half of them absent
    rng = np.random.default_rng(5)
    probe = d_keys[torch.from_numpy(rng.permutation(entries)[:65536]).cuda()].contiguous()
    probe[::2] = torch.from_numpy(rng.integers(0, 256, size=(32768, 16), dtype=np.uint8)).cuda()
    d_out = torch.empty((65536, 16), dtype=torch.uint8, device="cuda")
    d_found = torch.empty(65536, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def lookup() -> None:
        assert lib.map_lookup_batch_device(vm.h, m, probe.data_ptr(), 65536, d_out.data_ptr(), d_found.data_ptr(), s) == 0

    def restore_compacted(img):
        def f() -> None:
            restore(img)
            compact()
        return f

    t64, t512 = tables["tombstones_65536"], tables["tombstones_524288"]
    calls = {
        "compact_after_65536": series(compact, lambda: restore(t64)),
        "compact_after_524288": series(compact, lambda: restore(t512)),
        "count_only_524288": series(lambda: compact(CC.COUNT_ONLY), lambda: restore(t512)),
        "lookup_65536_with_524288_tombstones": series(lookup, lambda: restore(t512)),
        "lookup_65536_after_compaction": series(lookup, restore_compacted(t512)),
        "c5_batch_with_524288_tombstones": series(batch, lambda: restore(t512)),
        "c5_batch_after_compaction": series(batch, restore_compacted(t512)),
    }
    restore(t512)
    lookup()
    torch.cuda.synchronize()
    found_before = d_found.clone()
    compact()
    lookup()
    torch.cuda.synchronize()
    assert torch.equal(found_before, d_found) and int(d_found.sum()) > 10000, "the lookups differ after the compaction"

    # ---- today's route: a host visit, then the re-upload by the next device call (wall clock), beside the call
    today, device = [], []
    for rep in range(2 + 5):
        restore(t64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert vm.map_count(m) == entries - 65536
        t1 = time.perf_counter()
        compact(CC.COUNT_ONLY)  # the next device call uploads the rebuilt mirror
        t2 = time.perf_counter()
        restore(t64)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        compact()
        t4 = time.perf_counter()
        if rep >= 2:
            today.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3))
            device.append((t4 - t3) * 1e3)
    t_old, t_visit, t_new = float(np.median([t[0] for t in today])), float(np.median([t[1] for t in today])), float(np.median(device))

    # ---- one run of kMcMaxRun slots in a table of 16,384 (tests/mapcompact_cases.py run_long's layout)
    keys = CC.keys_at(CC.LONG_CAP, [CC.LONG_START] + [CC.LONG_START + j - 1 for j in range(1, CC.MAX_RUN)])
    img = np.zeros(vm.map_state_bytes(small), dtype=np.uint8)
    rec, ivals = CC.views(vm, small, img)
    at = CC.LONG_START + np.arange(CC.MAX_RUN)
    rec[at, 0], rec[at, 1], ivals[at] = CC.SLOT_FULL, keys.view(np.uint64).reshape(-1), 7
    rec[at[1], 0], ivals[at[1]] = CC.SLOT_TOMB, 0
    img[-8:-4] = np.array([CC.MAX_RUN - 1], dtype=np.uint32).view(np.uint8)
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()

    def compact_small():
        info = N.MapCompactInfo()
        assert lib.map_compact(vm.h, small, 0, C.byref(info), s) == 0
        assert (info.tombstones, info.moved, info.longest_run, info.via_host) == (1, CC.MAX_RUN - 2, CC.MAX_RUN, 0)

    calls["one_run_of_kMcMaxRun"] = series(compact_small, lambda: lib.map_state_import(vm.h, small, d_img.data_ptr(), s))

    out = {"map": {"type": "HASH", "key_size": 16, "value_size": 16, "max_entries": W.C5_MAX, "entries": entries, "slots": 2 * W.C5_MAX},
           "batch_packets": n, "kMcMaxRun": CC.MAX_RUN,
           "tables": {k: dict(zip(("tombstones", "moved", "longest_run", "via_host"), v)) for k, v in infos.items()},
           "checked_against_the_model": not a.no_model, "calls": calls,
           "today": {"what": "xe_map_count (download, rebuild of the mirror) + the upload by the next device call (wall), beside xe_map_compact "
                             "on the same table with 65,536 tombstones (wall)",
                     "calls": len(today), "host_visit_median_ms": t_visit, "host_visit_and_upload_median_ms": t_old, "map_compact_median_ms": t_new},
           "acceptance": {"today_ms": t_old, "map_compact_ms": t_new, "today_over_map_compact": t_old / t_new, "faster": t_new < t_old}}
    vm.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
