"""Cases and the numpy reference for the verdict dispatch (include/xdpemu_io.h, output side), shared by
the host-simulation tests (test_dispatch.py) and the device tests (test_dispatch_gpu.py). The outputs are
fully determined, so every comparison is for exact equality."""
import ctypes as C

import numpy as np

from gobpfld_amd import _native as N
from gobpfld_amd.dispatch import Dispatcher

T = N.XE_DISPATCH_TILE
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
DESC, RESULT, _ = N.np_dtypes()
INVAL = -22

GATHER_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1514]
SRC_ALIGN = [0, 1, 8, 15]
DST_ALIGN = [0, 1]
FRAME, SLOT = 2048, 1600
ROOMS = [1600, 65]  # frame_room: every length fits / the kernel's form for short frames, where 1514 bytes do not fit
UNALIGNED_SIZES = [65, T + 1, 3 * T + 17]  # less than a tile, a tile and one packet, several tiles and a partial one
STRIDE_ROOMS = [300, 64]  # check_gather_stride: the 16-lane form, the 4-lane form


class Mem:
    """Buffers where the library under test reads them: numpy arrays (64-byte aligned) for the host
    simulation, torch device tensors for the product."""

    def __init__(self, on_device: bool):
        self.on_device = on_device

    def put(self, arr: np.ndarray, offset: int = 0):
        """offset: the bytes start that far past a 16-byte boundary (a view of a larger buffer)."""
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        if self.on_device:
            import torch
            t = torch.empty(offset + max(b.size, 64), dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            t[offset:offset + b.size].copy_(torch.from_numpy(b.copy()))
            return t[offset:]
        raw = np.zeros(offset + b.size + 128, np.uint8)
        off = (-raw.ctypes.data) % 64 + offset
        out = raw[off:off + max(b.size, 64)]
        out[:b.size] = b
        return out

    def ptr(self, buf) -> int:
        return buf.data_ptr() if self.on_device else buf.ctypes.data

    def get(self, buf, nbytes: int) -> np.ndarray:
        if self.on_device:
            import torch
            torch.cuda.synchronize()
            return buf[:nbytes].cpu().numpy()
        return buf[:nbytes].copy()


def reference(ver, status=None):
    """(order, offset[6], invalid, failed) of the issue's numpy statement."""
    v = ver.astype(np.uint32)
    cls = np.where(v <= 4, v, 0).astype(np.uint8)
    st = np.zeros(len(v), np.uint8) if status is None else status
    cls[st != 0] = 0
    order = np.argsort(cls, kind="stable")
    offset = np.concatenate([[0], np.cumsum(np.bincount(cls, minlength=5))]).astype(np.int64)
    return order, offset.tolist(), int(((v > 4) & (st == 0)).sum()), int((st != 0).sum())


def random_desc(n, rng):
    d = np.zeros(n, DESC)
    d["addr"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n, dtype=np.uint64)
    d["len"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    d["options"] = np.arange(n, dtype=np.uint32)
    return d


def mixes(n, rng):
    """name -> (verdicts, statuses)"""
    ok = np.zeros(n, np.uint8)
    out = {f"all{c}": (np.full(n, c, np.uint32), ok) for c in range(5)}
    out["alt31"] = (np.where(np.arange(n) % 2 == 0, 3, 1).astype(np.uint32), ok)
    out["uniform"] = (rng.choice(np.array([0, 1, 2, 3, 4, 5, 0xFFFFFFFF], np.uint32), size=n), ok)
    v = rng.integers(0, 5, size=n, dtype=np.uint32)
    bad = rng.random(n) < 0.10
    v[bad] = 3
    out["failed10"] = (v, np.where(bad, rng.integers(1, 5, size=n), 0).astype(np.uint8))
    return out


def results_of(status):
    r = np.zeros(len(status), RESULT)
    r["status"] = status
    r["r0_kind"], r["code"], r["pc"], r["r0"] = 0xFF, 0xFFFF, 0xFFFFFFFF, -1  # only the status byte may count
    return r


def check_dispatch(lib, on_device, n, names=None, seed=1, ver_offset=0):
    """ver_offset (in verdicts, 4 bytes each): the verdict array starts that far past a 16-byte boundary, as
    the API allows; the count kernel then reads it with scalar loads (xe_dispatch.hip load_rows_packed)."""
    rng = np.random.default_rng(seed + n)
    mem, dsp = Mem(on_device), Dispatcher(lib, on_device=on_device)
    desc = random_desc(n, rng)
    d_desc = mem.put(desc)
    for name, (ver, status) in mixes(n, rng).items():
        if names is not None and name not in names:
            continue
        d_ver, d_res = mem.put(ver, offset=4 * ver_offset), mem.put(results_of(status))
        assert mem.ptr(d_ver) % 16 == (4 * ver_offset) % 16
        for with_results in (False, True):
            order, offset, invalid, failed = reference(ver, status if with_results else None)
            for with_index in (False, True):
                part = dsp.run(mem.ptr(d_desc), mem.ptr(d_ver), n, d_results=mem.ptr(d_res) if with_results else 0,
                               want_index=with_index)
                c = part.counts()
                what = f"n={n} mix={name} results={with_results} index={with_index}"
                assert (c.offset, c.invalid, c.failed) == (offset, invalid, failed), what
                assert (part.desc_host() == desc[order]).all(), what
                if with_index:
                    assert (part.index_host() == order).all(), what
                else:
                    assert part.index_host() is None
                assert sum(c.sizes) == n and [len(part.segment(k)[0]) for k in range(5)] == c.sizes, what


def check_errors(lib, on_device):
    mem = Mem(on_device)
    n = 300
    rng = np.random.default_rng(5)
    desc, ver = mem.put(random_desc(n + 1, rng)), mem.put(np.full(n, 2, np.uint32))
    out, counts = mem.put(np.zeros(n, DESC)), mem.put(np.zeros(8, np.uint32))
    need = C.c_uint64()
    assert lib.dispatch_scratch_bytes(n, C.byref(need)) == 0 and need.value > 0
    assert lib.dispatch_scratch_bytes(n, None) == INVAL
    scratch = mem.put(np.zeros(need.value, np.uint8))
    p = mem.ptr

    def call(d=p(desc), v=p(ver), o=p(out), c=p(counts), s=p(scratch), sb=need.value):
        return lib.dispatch_device(d or None, v or None, None, n, o or None, None, c or None, s or None, sb, None)

    assert call() == 0
    assert call(d=0) == INVAL and call(v=0) == INVAL and call(o=0) == INVAL and call(c=0) == INVAL and call(s=0) == INVAL
    assert call(sb=need.value - 1) == INVAL and call(sb=0) == INVAL
    assert call(o=p(desc)) == INVAL            # in place
    assert call(o=p(desc) + 16) == INVAL       # shifted by one descriptor
    assert call(d=p(desc) + 16, o=p(desc)) == INVAL  # the other way round
    rej = mem.put(np.zeros(1, np.uint32))
    assert lib.gather_device(p(desc), 64, p(out), p(counts), 5, 1, p(desc), 64, p(out), 64, p(out), p(rej), None) == INVAL
    assert lib.gather_device(p(desc), 64, p(out), None, 3, 1, p(desc), 64, p(out), 64, p(out), p(rej), None) == INVAL
    assert lib.gather_device(p(desc), 64, p(out), p(counts), 3, 1, p(desc), 64, p(out), 64, p(out), None, None) == INVAL
    # n == 0: only the counts record is needed, and it is zeroed
    dirty = mem.put(np.full(8, 0xABABABAB, np.uint32))
    assert lib.dispatch_device(None, None, None, 0, None, None, p(dirty), None, 0, None) == 0
    assert not mem.get(dirty, 32).any()
    z = C.c_uint64(1)
    assert lib.dispatch_scratch_bytes(0, C.byref(z)) == 0 and z.value == 0

    # alignment: descriptors and scratch 16 bytes, verdicts, index and counts 4, frames 8. A pointer that
    # is off is refused before anything runs: the outputs keep what they held.
    PAT = 0xEE
    o_desc, o_idx, o_cnt = (mem.put(np.full(k, PAT, np.uint8)) for k in ((n + 1) * 16, (n + 1) * 4, 64))
    ver1 = mem.put(np.full(n + 1, 2, np.uint32))
    scratch1 = mem.put(np.zeros(need.value + 16, np.uint8))  # (room behind a shifted pointer: only the alignment is off)
    args = dict(d=p(desc), v=p(ver1), o=p(o_desc), i=p(o_idx), c=p(o_cnt), s=p(scratch1))

    def dispatch(**shift):
        a = {k: v + shift.get(k, 0) for k, v in args.items()}
        return lib.dispatch_device(a["d"], a["v"], None, n, a["o"], a["i"], a["c"], a["s"], need.value, None)

    for shift in (dict(d=8), dict(o=8), dict(v=2), dict(i=2), dict(s=8), dict(c=2)):
        assert dispatch(**shift) == INVAL, shift
    for buf in (o_desc, o_idx, o_cnt):
        assert (mem.get(buf, len(buf)) == PAT).all(), "a refused dispatch wrote to its outputs"
    assert dispatch(v=4, i=4, c=4) == 0  # what the API allows
    order, offset, _, _ = reference(np.full(n, 2, np.uint32))
    assert mem.get(o_cnt, 36)[4:].view(np.uint32)[:6].tolist() == offset
    assert (mem.get(o_desc, n * 16).view(DESC) == mem.get(desc, n * 16).view(DESC)).all()

    # the gather, over the partition just written (class 2 holds all n packets)
    src = mem.put(rng.integers(0, 256, size=4096, dtype=np.uint8))
    small = np.zeros(n, DESC)
    small["addr"], small["len"] = np.arange(n) * 8, 8
    sorted_desc = mem.put(small)
    counts2 = mem.put(np.array([0, 0, 0, n, n, n, 0, 0], np.uint32))
    frames = mem.put(np.arange(n + 1, dtype=np.uint64) * 16)
    g_dst, g_out, g_rej = (mem.put(np.full(k, PAT, np.uint8)) for k in (n * 16 + 64, (n + 1) * 16, 64))
    gargs = dict(s=p(sorted_desc), o=p(g_out), f=p(frames), c=p(counts2), r=p(g_rej))

    def gather(**shift):
        a = {k: v + shift.get(k, 0) for k, v in gargs.items()}
        return lib.gather_device(p(src), 4096, a["s"], a["c"], 2, n, a["f"], 64, p(g_dst), n * 16 + 64, a["o"], a["r"], None)

    for shift in (dict(s=8), dict(o=8), dict(f=4), dict(c=2), dict(r=2)):
        assert gather(**shift) == INVAL, shift
    for buf in (g_dst, g_out, g_rej):
        assert (mem.get(buf, len(buf)) == PAT).all(), "a refused gather wrote to its outputs"
    assert gather() == 0
    assert mem.get(g_rej, 4).view(np.uint32)[0] == 0
    want = np.full(n * 16 + 64, PAT, np.uint8)
    want[:n * 16].reshape(n, 16)[:, :8] = mem.get(src, n * 8).reshape(n, 8)
    assert (mem.get(g_dst, n * 16 + 64) == want).all()


def gather_case(rng, room):
    """A batch whose class-3 packets cover the length x alignment matrix and the bounds cases, each
    followed by a class-1 packet so that the class-3 segment does not start at 0.
    Returns (src, src_len, desc, verdicts, frames, dst_len, accepted) with `accepted` per class-3 packet."""
    tx = []  # (addr, len, frame, ok)
    slot = 0
    for ln in GATHER_LENS:
        for sa in SRC_ALIGN:
            for da in DST_ALIGN:
                tx.append([slot * SLOT + sa, ln, len(tx) * FRAME + da, ln <= room])
                slot += 1
    src_len = slot * SLOT + 40
    nframes = len(tx) + 7
    dst_len = nframes * FRAME - 100
    k = len(tx)
    tx.append([src_len - 8, 8, k * FRAME, True])                      # ends exactly at src_len
    tx.append([src_len - 4, 8, (k + 1) * FRAME, False])               # one past src_len
    tx.append([(1 << 64) - 8, 16, (k + 2) * FRAME, False])            # addr + len wraps
    tx.append([0, room + 1, (k + 3) * FRAME, False])                  # longer than the frame's room
    tx.append([SLOT, room, (k + 4) * FRAME, True])                    # exactly the room
    tx.append([16, 8, dst_len - 4, False])                            # frame past dst_len
    tx.append([32, 8, dst_len - 8, True])                             # ends exactly at dst_len
    src = rng.integers(0, 256, size=src_len, dtype=np.uint8)
    desc = np.zeros(2 * len(tx), DESC)
    ver = np.ones(2 * len(tx), np.uint32)
    for i, (a, ln, _, _) in enumerate(tx):
        desc[2 * i] = (a, ln, 7)
        ver[2 * i] = 3
        desc[2 * i + 1] = ((1 << 64) - 1, 0xFFFFFFFF, 9)  # never followed: class 1 is not gathered
    frames = np.array([t[2] for t in tx], np.uint64)
    return src, src_len, desc, ver, frames, dst_len, tx


def check_gather(lib, on_device, room):
    rng = np.random.default_rng(11)
    src, src_len, desc, ver, frames, dst_len, tx = gather_case(rng, room)
    mem, dsp = Mem(on_device), Dispatcher(lib, on_device=on_device)
    d_src, d_desc, d_ver, d_frames = mem.put(src), mem.put(desc), mem.put(ver), mem.put(frames)
    part = dsp.run(mem.ptr(d_desc), mem.ptr(d_ver), len(desc))
    seg = len(tx)
    assert part.counts().sizes == [0, seg, 0, seg, 0]
    if on_device:
        assert mem.ptr(d_src) % 16 == 0
    for max_count in (seg + 5, seg - 3, None, 0):
        d_dst = mem.put(np.full(dst_len, 0xEE, np.uint8))
        assert mem.ptr(d_dst) % 16 == 0
        g = dsp.gather(mem.ptr(d_src), src_len, part, N.ACT_TX, mem.ptr(d_frames), room, mem.ptr(d_dst), dst_len,
                       max_count=max_count)
        take = seg if max_count is None else min(seg, max_count)
        want = np.full(dst_len, 0xEE, np.uint8)
        want_desc = np.zeros(take, DESC)
        rejected = 0
        for k, (a, ln, f, ok) in enumerate(tx[:take]):
            if ok:
                want[f:f + ln] = src[a:a + ln]
            want_desc[k] = (f, ln if ok else 0, 0)
            rejected += not ok
        assert g.rejected() == rejected, max_count
        assert (g.desc_host(take) == want_desc).all(), max_count
        assert (mem.get(d_dst, dst_len) == want).all(), max_count
        assert (mem.get(d_src, src_len) == src).all()
    # a counts record that is not one the dispatch wrote selects nothing
    bad = mem.put(np.array([0, 5, 5, 4, 9, 9, 0, 0], np.uint32))
    d_dst = mem.put(np.full(dst_len, 0xEE, np.uint8))
    rej, out = mem.put(np.full(1, 77, np.uint32)), mem.put(np.zeros(seg, DESC))
    assert lib.gather_device(mem.ptr(d_src), src_len, part.d_desc, mem.ptr(bad), 2, seg, mem.ptr(d_frames), room,
                             mem.ptr(d_dst), dst_len, mem.ptr(out), mem.ptr(rej), None) == 0
    assert (mem.get(d_dst, dst_len) == 0xEE).all() and mem.get(rej, 4).view(np.uint32)[0] == 0


# xe_dispatch.hip xe_launch_gather: at most 8192 workgroups of 256 threads, a group of 16 lanes per packet
# (4 lanes when frame_room <= 256), so 8192 x 16 (x 64) packets are in flight before a group strides on to
# a second packet, with that packet's descriptor and frame loaded ahead of the first one's bytes.
GATHER_MAX_BLOCKS, GATHER_SHORT_ROOM = 8192, 256
STRIDE_EXTRA = 777


def check_gather_stride(lib, on_device, room):
    per = 256 // (4 if room <= GATHER_SHORT_ROOM else 16)
    count = GATHER_MAX_BLOCKS * per + STRIDE_EXTRA
    rng = np.random.default_rng(room)
    src_len = 1 << 20
    src = rng.integers(0, 256, size=src_len, dtype=np.uint8)
    desc = np.zeros(count, DESC)
    desc["addr"] = rng.integers(0, src_len - room, size=count, dtype=np.uint64)  # addr % 16: every residue
    desc["len"] = rng.integers(0, room + 1, size=count, dtype=np.uint32)
    desc["options"] = 5
    bad = rng.random(count) < 1e-3
    bad[[0, GATHER_MAX_BLOCKS * per - 1, GATHER_MAX_BLOCKS * per, count - 1]] = [False, True, True, False]
    too_long = bad & (rng.random(count) < 0.5)
    desc["len"][too_long] = room + 1
    desc["addr"][bad & ~too_long] = src_len + 1 + rng.integers(0, 1 << 40, size=int((bad & ~too_long).sum()), dtype=np.uint64)
    assert len(np.unique(desc["addr"][:4096] % 16)) == 16 and 0 < bad.sum() < count // 500
    stride = (room + 15) // 16 * 16 + 16
    k = np.arange(count, dtype=np.uint64)
    frames = k * np.uint64(stride) + k % np.uint64(3)
    dst_len = count * stride + 16
    ver = np.full(count, 3, np.uint32)

    # the expected destination, without a loop over the packets: flat byte index -> (packet, offset in it)
    # (int32 throughout: dst_len and the bytes moved are far below 2^31)
    lens = np.where(bad, 0, desc["len"]).astype(np.int32)
    pid = np.repeat(np.arange(count, dtype=np.int32), lens)
    within = np.arange(len(pid), dtype=np.int32) - np.repeat(np.cumsum(lens, dtype=np.int32) - lens, lens)
    to = frames.astype(np.int32)[pid] + within
    frm = np.where(bad, 0, desc["addr"]).astype(np.int32)[pid] + within
    assert dst_len < 1 << 31 and len(pid) == int(lens.sum(dtype=np.int64)) and to.dtype == np.int32
    want_desc = np.zeros(count, DESC)
    want_desc["addr"], want_desc["len"] = frames, lens

    mem, dsp = Mem(on_device), Dispatcher(lib, on_device=on_device)
    d_src, d_desc, d_ver, d_frames = mem.put(src), mem.put(desc), mem.put(ver), mem.put(frames)
    part = dsp.run(mem.ptr(d_desc), mem.ptr(d_ver), count, want_index=False)
    assert part.counts().sizes == [0, 0, 0, count, 0]
    for max_count in (None, count - 5000):  # the second: the last turn of the grid stride is a partial one
        take = count if max_count is None else max_count
        d_dst = mem.put(np.full(dst_len, 0xEE, np.uint8))
        g = dsp.gather(mem.ptr(d_src), src_len, part, N.ACT_TX, mem.ptr(d_frames), room, mem.ptr(d_dst), dst_len,
                       max_count=max_count)
        want = np.full(dst_len, 0xEE, np.uint8)
        sel = pid < take
        want[to[sel]] = src[frm[sel]]
        what = f"room={room} max_count={max_count}"
        assert g.rejected() == int(bad[:take].sum()), f"{what}: rejected differs"
        rows = g.desc_host(take)
        assert (rows == want_desc[:take]).all(), f"{what}: out_desc differs from row {np.flatnonzero(rows != want_desc[:take])[:1]}"
        got = mem.get(d_dst, dst_len)
        assert (got == want).all(), f"{what}: destination differs at bytes {np.flatnonzero(got != want)[:8].tolist()}"
        assert (mem.get(d_src, src_len) == src).all()
