"""Verdict dispatch: the output side of a batch (include/xdpemu_io.h).

`xe_run_batch_device` leaves one uint32 verdict per packet; a forwarder works with lists. The
`Dispatcher` partitions a batch's descriptors by XDP action on the device (stable: packet order is
kept within an action) and gathers one action's packets into frames the caller chose:

    dsp = Dispatcher()                                   # product library, torch device buffers
    vm.run_batch_device(umem.data_ptr(), umem.numel(), desc.data_ptr(), n, d_verdicts=ver.data_ptr())
    part = dsp.run(desc.data_ptr(), ver.data_ptr(), n)   # xe_dispatch_device
    tx = dsp.gather(umem.data_ptr(), umem.numel(), part, N.ACT_TX, frames.data_ptr(), 2048,
                    txbuf.data_ptr(), txbuf.numel(), max_count=len(frames))
    part.counts().sizes                                  # packets per action (a 32-byte copy back)

Pointers go in as ints, the way `VM.run_batch_device` takes them. The same class drives the host
simulation (tests): buffers are then numpy arrays and the pointers host addresses. A Dispatcher owns
its workspace, so use one per stream.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N


class DispatchError(RuntimeError):
    pass


@dataclass
class Counts:
    """xe_dispatch_counts on the host."""
    offset: list  # class c occupies [offset[c], offset[c + 1]); offset[5] == n
    invalid: int  # verdict > 4 (status OK): sent to class 0
    failed: int   # status != XE_ST_OK: sent to class 0

    @property
    def sizes(self) -> list:
        return [self.offset[c + 1] - self.offset[c] for c in range(N.ACT_COUNT)]


class _Buffers:
    """Byte buffers of one kind: torch device tensors for the product, numpy arrays for the host simulation."""

    def __init__(self, on_device: bool):
        self.on_device = on_device
        if on_device:
            import torch
            self.torch = torch

    def alloc(self, nbytes: int):
        if self.on_device:
            return self.torch.empty(max(nbytes, 16), dtype=self.torch.uint8, device="cuda")
        return np.zeros(max(nbytes, 16), dtype=np.uint8)

    def ptr(self, buf) -> int:
        return buf.data_ptr() if self.on_device else buf.ctypes.data

    def host(self, buf, stream: int) -> np.ndarray:
        """The bytes on the host, ordered after the work queued on `stream`."""
        if not self.on_device:
            return buf
        torch = self.torch
        if not stream:
            return buf.cpu().numpy()
        s = torch.cuda.ExternalStream(stream)
        with torch.cuda.stream(s):
            h = buf.to("cpu", non_blocking=True)
        s.synchronize()
        return h.numpy()


class Dispatched:
    """One batch's partition. `desc` / `index` are the whole output arrays (device tensors of bytes /
    int32 on the product; a structured array / uint32 in the host simulation); `counts()`,
    `segment()` and the `*_host()` forms wait for the stream and copy back."""

    def __init__(self, bufs: _Buffers, n: int, desc, index, counts, stream: int):
        self._b, self.n, self._desc, self._index, self._counts, self.stream = bufs, n, desc, index, counts, stream
        self._host_counts: Counts | None = None

    @property
    def d_desc(self) -> int:
        return self._b.ptr(self._desc)

    @property
    def d_index(self) -> int:
        return self._b.ptr(self._index) if self._index is not None else 0

    @property
    def d_counts(self) -> int:
        return self._b.ptr(self._counts)

    @property
    def desc(self):
        d = self._desc[:self.n * 16]
        return d.view(-1, 16) if self._b.on_device else d.view(N.np_dtypes()[0])

    @property
    def index(self):
        if self._index is None:
            return None
        i = self._index[:self.n * 4]
        return i.view(self._b.torch.int32) if self._b.on_device else i.view(np.uint32)

    def counts(self) -> Counts:
        if self._host_counts is None:
            w = self._b.host(self._counts[:32], self.stream).view(np.uint32)
            self._host_counts = Counts([int(x) for x in w[:6]], int(w[6]), int(w[7]))
        return self._host_counts

    def segment(self, cls: int):
        """(descriptors, packet indices or None) of one class: views of `desc` and `index`."""
        c = self.counts()
        lo, hi = c.offset[cls], c.offset[cls + 1]
        return self.desc[lo:hi], (self.index[lo:hi] if self._index is not None else None)

    def desc_host(self) -> np.ndarray:
        return self._b.host(self._desc[:self.n * 16], self.stream).view(N.np_dtypes()[0])

    def index_host(self) -> np.ndarray | None:
        return None if self._index is None else self._b.host(self._index[:self.n * 4], self.stream).view(np.uint32)


class Gathered:
    """One gather's outputs: `out_desc` has room for the requested packets; `rejected()` and
    `desc_host()` wait for the stream."""

    def __init__(self, bufs: _Buffers, room: int, out_desc, rejected, stream: int):
        self._b, self.room, self._desc, self._rej, self.stream = bufs, room, out_desc, rejected, stream

    @property
    def d_out_desc(self) -> int:
        return self._b.ptr(self._desc)

    def rejected(self) -> int:
        return int(self._b.host(self._rej[:4], self.stream).view(np.uint32)[0])

    def desc_host(self, count: int | None = None) -> np.ndarray:
        k = self.room if count is None else min(count, self.room)
        return self._b.host(self._desc[:k * 16], self.stream).view(N.np_dtypes()[0])


class Dispatcher:
    def __init__(self, lib: N.Lib | None = None, on_device: bool | None = None):
        self.lib = lib or N.product()
        for name in ("dispatch_scratch_bytes", "dispatch_device", "gather_device"):
            if not self.lib.has(name):
                raise DispatchError(f"{self.lib.path.name} has no xe_{name}")
        if on_device is None:
            on_device = self.lib.path.resolve() in (N.PRODUCT_LIB.resolve(), N.TUNING_LIB.resolve())
        self._b = _Buffers(on_device)
        self._scratch = None
        self._scratch_bytes = 0

    def scratch_bytes(self, n: int) -> int:
        b = C.c_uint64()
        if self.lib.dispatch_scratch_bytes(n, C.byref(b)):
            raise DispatchError("xe_dispatch_scratch_bytes")
        return b.value

    def run(self, d_desc: int, d_verdicts: int, n: int, d_results: int = 0, want_index: bool = True,
            stream: int = 0, into: Dispatched | None = None) -> Dispatched:
        """Partition the batch (xe_dispatch_device), stream-ordered. `into`: an earlier result whose
        buffers are reused when they are large enough (a serving loop allocates once)."""
        need = self.scratch_bytes(n)
        if need > self._scratch_bytes:
            self._scratch, self._scratch_bytes = self._b.alloc(need), need
        b = self._b
        reuse = into is not None and len(into._desc) >= n * 16 and (not want_index or (into._index is not None and len(into._index) >= n * 4))
        if reuse:
            desc, index, counts = into._desc, into._index if want_index else None, into._counts
        else:
            desc, index, counts = b.alloc(n * 16), b.alloc(n * 4) if want_index else None, b.alloc(32)
        rc = self.lib.dispatch_device(d_desc or None, d_verdicts or None, d_results or None, n, b.ptr(desc),
                                      b.ptr(index) if index is not None else None, b.ptr(counts),
                                      b.ptr(self._scratch) if self._scratch is not None else None, self._scratch_bytes,
                                      stream or None)
        if rc:
            raise DispatchError(f"xe_dispatch_device failed (rc={rc})")
        return Dispatched(b, n, desc, index, counts, stream)

    def gather(self, d_src: int, src_len: int, part: Dispatched, cls: int, d_frames: int, frame_room: int,
               d_dst: int, dst_len: int, max_count: int | None = None, stream: int | None = None) -> Gathered:
        """Copy class `cls`'s packets into the frames listed at d_frames (xe_gather_device); the segment
        bounds are read on the device. max_count: the entries d_frames holds; None takes the class's
        size from the counts (a copy back)."""
        stream = part.stream if stream is None else stream
        if max_count is None:
            max_count = part.counts().sizes[cls]
        b = self._b
        out, rej = b.alloc(max_count * 16), b.alloc(4)
        rc = self.lib.gather_device(d_src or None, src_len, part.d_desc, part.d_counts, cls, max_count, d_frames or None,
                                    frame_room, d_dst or None, dst_len, b.ptr(out), b.ptr(rej), stream or None)
        if rc:
            raise DispatchError(f"xe_gather_device failed (rc={rc})")
        return Gathered(b, max_count, out, rej, stream)
