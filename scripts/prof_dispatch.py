#!/usr/bin/env python3
"""Time the verdict dispatch (xe_dispatch_device) and the TX gather (xe_gather_device) at the bench's own
size, 16,777,216 x 64 B C2 packets (BASELINE configs[1]), against what a caller did before they existed:
the verdicts copied to pinned host memory and partitioned with numpy.

    python scripts/prof_dispatch.py --out profiles/dispatch/dispatch.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/prof_dispatch.py --trace-run   # kernel times

Dispatch is timed on two inputs, the verdicts the C2 kernel produced (two classes) and a synthetic
uniform five-class mix, each without and with d_results; the gather takes the synthetic mix's TX class
into dense 64-byte frames, in both forms of its kernel (4 and 16 lanes per packet). Every output is
compared with numpy for equality at this size before anything is timed. Times are device events around single calls, after warm-up, the variants and the host path
alternating in one run; each variant's window is at least --window seconds of device time.
Algorithmic bytes per packet: dispatch reads 4 (verdict) + 16 (descriptor) and writes 16 + 4; with results
it uses 1 more byte, for which the 16-byte stride makes it fetch the whole 16. The gather reads 16 + 8 + len
and writes len + 16 per packet. Shares are of the 6.3 TB/s achievable HBM rate.
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


def partition(ver: np.ndarray, status: np.ndarray | None, descs: np.ndarray):
    """The numpy stable partition: (out_desc, out_index, offset[6])."""
    cls = np.where(ver <= 4, ver, 0).astype(np.uint8)
    if status is not None:
        cls[status != 0] = 0
    order = np.argsort(cls, kind="stable")
    offset = np.concatenate([[0], np.cumsum(np.bincount(cls, minlength=5))])
    return descs[order], order.astype(np.uint32), offset


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16_777_216)
    ap.add_argument("--window", type=float, default=0.5, help="least device seconds timed per variant")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-run", action="store_true", help="a short run for a kernel trace: 20 calls per variant, no host path")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("prof_dispatch: no GPU")
    from gobpfld_amd import _native as N
    from gobpfld_amd import workloads as W
    from gobpfld_amd.dispatch import Dispatcher
    from gobpfld_amd.emulator import VM, Settings

    n = a.n
    umem, descs = W.build_batch("c2", 0, n)
    d_umem = torch.from_numpy(umem).cuda()
    d_desc = torch.from_numpy(descs.view(np.uint8)).cuda()
    d_res = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    d_c2 = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    vm = VM(Settings())
    W.setup_vm(vm, "c2")
    for _ in range(3):
        st = vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_results=d_res.data_ptr(),
                                 d_verdicts=d_c2.data_ptr(), stream=s)
    c2_kernel_ms = st["kernel_ms"]
    rng = np.random.default_rng(0)
    synth = rng.integers(0, 5, size=n, dtype=np.uint32)
    d_synth = torch.from_numpy(synth.view(np.int32)).cuda()
    h_c2 = d_c2.cpu().numpy().view(np.uint32)
    status = d_res.cpu().numpy().view(N.np_dtypes()[1])["status"].copy()

    dsp = Dispatcher()
    inputs = {"c2": (d_c2, h_c2), "uniform5": (d_synth, synth)}
    variants = [(name, res) for res in (False, True) for name in inputs]  # (input, with d_results)
    parts = {}

    def dispatch(name, res):
        key = (name, res)
        parts[key] = dsp.run(d_desc.data_ptr(), inputs[name][0].data_ptr(), n, d_results=d_res.data_ptr() if res else 0,
                             stream=s, into=parts.get(key))
        return parts[key]

    for name, res in variants:  # equality with numpy at this size, before any timing
        p = dispatch(name, res)
        want_desc, want_index, want_off = partition(inputs[name][1], status if res else None, descs)
        assert p.counts().offset == want_off.tolist(), (name, res)
        assert (p.index_host() == want_index).all() and (p.desc_host() == want_desc).all(), (name, res)
        del want_desc, want_index

    tx = parts[("uniform5", False)]
    ntx = tx.counts().sizes[N.ACT_TX]
    d_frames = (torch.arange(ntx, dtype=torch.int64, device="cuda") * 64)
    d_dst = torch.empty(ntx * 64, dtype=torch.uint8, device="cuda")

    def gather(room):  # frame_room picks the kernel's form: 4 lanes per packet up to 256 bytes, else 16
        return dsp.gather(d_umem.data_ptr(), d_umem.numel(), tx, N.ACT_TX, d_frames.data_ptr(), room, d_dst.data_ptr(),
                          d_dst.numel(), max_count=ntx, stream=s)

    src_rows = torch.from_numpy((descs["addr"][synth == 3] // 64).astype(np.int64)).cuda()
    for room in (64, 2048):
        d_dst.fill_(0xEE)
        assert gather(room).rejected() == 0
        assert torch.equal(d_dst.view(ntx, 64), d_umem.view(n, 64)[src_rows]), "gathered bytes differ"
    del src_rows

    calls = {f"dispatch_{name}{'_results' if res else ''}": (lambda name=name, res=res: dispatch(name, res)) for name, res in variants}
    calls["gather_tx_uniform5_4lanes"] = lambda: gather(64)
    calls["gather_tx_uniform5_16lanes"] = lambda: gather(2048)

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    h_pin = torch.empty(n, dtype=torch.int32, pin_memory=True)

    def host_path(d_ver) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_pin.copy_(d_ver, non_blocking=True)
        torch.cuda.synchronize()
        partition(h_pin.numpy().view(np.uint32), None, descs)
        return (time.perf_counter() - t0) * 1e3

    for fn in calls.values():
        for _ in range(10):
            timed(fn)
    probe = {k: min(timed(fn) for _ in range(5)) for k, fn in calls.items()}
    blocks = 1 if a.trace_run else max(a.host_reps, 1)
    per_block = {k: 20 if a.trace_run else max(20, int(a.window * 1e3 / ms / blocks) + 1) for k, ms in probe.items()}
    times = {k: [] for k in calls}
    host = {"c2": [], "uniform5": []}
    for _ in range(blocks):
        if not a.trace_run:
            for name in host:
                host[name].append(host_path(inputs[name][0]))
        left = dict(per_block)
        while any(left.values()):  # the variants take turns
            for k, fn in calls.items():
                if left[k]:
                    times[k].append(timed(fn))
                    left[k] -= 1
    torch.cuda.synchronize()
    vm.close()
    if a.trace_run:
        print("trace run done:", {k: len(v) for k, v in times.items()})
        return

    out = {"n": n, "packet_bytes": 64, "hbm_achievable_tbs": HBM_TBS, "c2_emulation_kernel_ms": c2_kernel_ms,
           "tile": N.XE_DISPATCH_TILE, "classes_c2": parts[("c2", False)].counts().sizes,
           "classes_uniform5": tx.counts().sizes, "stages": {}, "host_path": {}}
    for name, v in host.items():
        out["host_path"][name] = {"what": "D2H of the verdicts into pinned memory + numpy stable partition (descriptors, indices, offsets)",
                                  "reps": len(v), "median_ms": float(np.median(v)), "min_ms": float(min(v))}
    for k, v in times.items():
        med = float(np.median(v))
        if k.startswith("dispatch"):
            per_packet = {"read": 4 + 16 + (1 if k.endswith("_results") else 0), "written": 16 + 4}
            total = n * (per_packet["read"] + per_packet["written"])
            inp = "c2" if "_c2" in k else "uniform5"
        else:
            per_packet = {"read": 16 + 8 + 64, "written": 64 + 16}
            total = ntx * (per_packet["read"] + per_packet["written"])
            inp = None
        tbs = total / (med * 1e-3) / 1e12
        row = {"calls": len(v), "window_s": float(sum(v)) * 1e-3, "median_ms": med, "mean_ms": float(np.mean(v)),
               "min_ms": float(min(v)), "p90_ms": float(np.percentile(v, 90)), "algorithmic_bytes_per_packet": per_packet,
               "packets": n if inp else ntx, "achieved_tbs": tbs, "share_of_hbm": tbs / HBM_TBS}
        if inp:
            row["host_over_device"] = out["host_path"][inp]["median_ms"] / med
            row["over_c2_emulation_kernel"] = med / c2_kernel_ms
        out["stages"][k] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
