"""Shared cases of the packet header window (gobpfld_amd/csrc/xe_interp.h hdr_rows, hdr_issue, lane_stage,
hdr_read_, in_window*, pkt_load, pkt_store; the per-program kernels' XE_HDR_LO / XE_HDR_HI from
xe_jit.cpp packet_read_range / emit_window): tests/test_window.py runs them on the host simulation,
tests/test_window_gpu.py on the product library with both engines.

No expected value comes from an emulator. A program here is a list of ops (`asm_ops`) with a numpy twin
(`twin`) that applies the same loads, stores and adds to the UMEM bytes of every packet:
a field is int.from_bytes(umem[a + off : a + off + size], "little"). Small batches also go through the
oracle and parity.assert_same (status, pc, steps, register records, the packet bytes left in the UMEM).
Every packet of every batch is compared.

The window in numbers (xe_interp.h): a lane's window is up to four 16-byte rows from the 16-byte aligned
address at or below packet byte XE_HDR_LO, so with XE_HDR_LO = 0 (the interpreter) a packet at 16-byte
phase p has its bytes [0, min(len, 64 - p)) in the window and everything above in HBM only. A packet
whose rows would run past the end of the UMEM is staged byte by byte instead (phase taken as 0)."""
from __future__ import annotations

import functools

import numpy as np

from gobpfld_amd.asm import JEQ, JGT, MUL, Asm
from gobpfld_amd.emulator import ENGINE_JIT, MAP_HASH, MODE_PARALLEL, MODE_SEQUENTIAL, VM, MapDef, Settings
from parity import assert_same, run_one

LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 59, 60, 61, 62, 63, 64, 65, 66, 79, 80, 81, 100)
SIZES = (1, 2, 4, 8)
PROBE_OFFS = range(0, 70)
M64 = (1 << 64) - 1
# read ranges [lo, hi) of the per-program kernels (one fold program each)
SHAPES = ((0, 1), (0, 14), (1, 2), (12, 28), (15, 17), (16, 32), (13, 62), (13, 63), (47, 64), (63, 64), (60, 100), (64, 72))
FULL = (0, 64)
MANY = 3 * (1 << 18) + 101  # packets of the many-chunks batch
SCHEDULES = (0, 977)


def _descs(addr, lens):
    from gobpfld_amd._native import np_dtypes
    d = np.zeros(len(addr), dtype=np_dtypes()[0])
    d["addr"], d["len"] = addr, lens
    return d


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def place(combos, start=0):
    """Addresses of packets (phase, length) one after another from `start`: each at the next 16-byte
    boundary + 16 + phase, so packets never overlap and have a foreign byte on each side. Returns the
    addresses and the first byte after the last packet."""
    addr, at = [], start
    for p, l in combos:
        at = ((at + 15) & ~15) + 16 + p
        addr.append(at)
        at += l
    return np.asarray(addr, dtype=np.int64), at


@functools.lru_cache(maxsize=None)
def layout(seed: int, tail_gap: int):
    """16 phases x LENS = 384 packets in a seeded shuffle (the lanes of one wave differ in phase and row
    count), in a UMEM of random bytes, gaps included, with `tail_gap` bytes after the last packet."""
    rng = np.random.default_rng(seed)
    combos = [(p, l) for p in range(16) for l in LENS]
    rng.shuffle(combos)
    addr, end = place(combos)
    umem = rng.integers(0, 256, size=end + tail_gap, dtype=np.uint8)
    return _frozen(umem, _descs(addr, [l for _, l in combos]))


@functools.lru_cache(maxsize=None)
def layout_many(seed: int):
    """MANY packets: the placement of layout(seed, 0) repeated every `pitch` bytes (a multiple of 16, so
    the phases stay), every byte of the UMEM random."""
    _, d = layout(seed, 0)
    a1, l1 = d["addr"].astype(np.int64), d["len"].astype(np.int64)
    pitch = (int(a1[-1] + l1[-1]) + 31) & ~15
    tiles = -(-MANY // len(a1))
    addr = (a1[None, :] + pitch * np.arange(tiles, dtype=np.int64)[:, None]).reshape(-1)[:MANY]
    lens = np.tile(l1, tiles)[:MANY]
    umem = np.random.default_rng(seed + 1).integers(0, 256, size=pitch * tiles, dtype=np.uint8)
    return _frozen(umem, _descs(addr, lens))


@functools.lru_cache(maxsize=None)
def layout_flat(seed: int, length: int = 100, copies: int = 2):
    """`copies` packets of `length` bytes at each of the 16 phases, shuffled (the write-through batches)."""
    rng = np.random.default_rng(seed)
    combos = [(p, length) for p in range(16)] * copies
    rng.shuffle(combos)
    addr, end = place(combos)
    umem = rng.integers(0, 256, size=end + 16, dtype=np.uint8)
    return _frozen(umem, _descs(addr, [length] * len(combos)))


TAIL_LAST = (1, 17, 33, 64)


@functools.lru_cache(maxsize=None)
def layout_tail(e: int, lo: int, hi: int):
    """64 + 16 + 1 packets in a UMEM whose length is e modulo 16. The last packet (length 1, 17, 33 or 64 in
    turn) ends exactly at the end of the UMEM. The 16 before it end in the last, partial 16-byte row (for
    e = 0 there is none: they end at the last byte), with lengths that put the end of their window
    [lo, min(len, hi)) there: the rows of their windows would run past the UMEM. These 17 packets overlap
    one another, which a read-only program does not notice. The first 64 are laid out as in `layout`."""
    rng = np.random.default_rng(1000 + e)
    combos = [(p, l) for p in range(16) for l in LENS]
    rng.shuffle(combos)
    combos = combos[:64]
    addr, end = place(combos)
    top = min(hi, lo + 64)
    tail_lens = [int(x) for x in np.linspace(lo + 1, top, 16).round()]
    total = ((end + 15) & ~15) + 16 * 8 + e  # room for the longest tail packet above the placed ones
    assert total % 16 == e and total - max(tail_lens + [64]) - 16 >= end
    tail_addr = [total - l - (j % e if e else 0) for j, l in enumerate(tail_lens)]
    for a, l in zip(tail_addr, tail_lens):  # the last window byte lies in the UMEM's last row
        assert a + l <= total and a + min(l, hi) - 1 >= ((total - 1) & ~15)
    last = TAIL_LAST[e % 4]
    addr = np.concatenate([addr, np.asarray(tail_addr + [total - last], dtype=np.int64)])
    lens = [l for _, l in combos] + tail_lens + [last]
    umem = rng.integers(0, 256, size=total, dtype=np.uint8)
    assert int((addr + np.asarray(lens)).max()) == total
    return _frozen(umem, _descs(addr, lens))


# ---------------------------------------------------------------- programs and their numpy twins
# ops: ("ld", off, size, guarded)   r0 = r0 * 31 + *(size*)(data + off); guarded: `goto out` if the field
#                                   does not fit below data_end
#      ("st", off, size, imm)       *(size*)(data + off) = imm            (ST, the immediate sign-extended)
#      ("stx", off, size, value)    *(size*)(data + off) = r6 = value     (STX)
#      ("add", off, size, value)    atomic add of r6 = value              (widths 4 and 8)
def asm_ops(ops) -> list[int]:
    a = Asm()
    a.ldx(4, 2, 1, 0).ldx(4, 3, 1, 4).mov64(0, 0)
    for kind, off, size, x in ops:
        if kind == "ld":
            if x:
                a.mov64(4, src=2).add64(4, off + size).jmp(JGT, 4, "out", src=3)
            a.ldx(size, 5, 2, off).alu64(MUL, 0, 31).add64(0, src=5)
        elif kind == "st":
            a.st(size, 2, off, x)
        elif kind == "stx":
            a.ld_imm64(6, x).stx(size, 2, off, 6)
        elif kind == "add":
            a.ld_imm64(6, x).xadd(size, 2, off, 6)
        else:
            raise ValueError(kind)
    a.label("out").exit()
    return a.assemble()


def _gather(mem, at, size):
    """int.from_bytes(mem[a : a + size], "little") for every a of `at`."""
    rows = np.lib.stride_tricks.sliding_window_view(mem, size)[at]
    return np.ascontiguousarray(rows).view(f"<u{size}").reshape(-1).astype(np.uint64)


def _scatter(mem, at, size, v):
    for b in range(size):
        mem[at + b] = (v >> np.uint64(8 * b)).astype(np.uint8)


def twin(ops, umem, descs):
    """What asm_ops(ops) leaves: R0 of every packet (uint64) and the UMEM bytes."""
    mem = umem.copy() if any(kind != "ld" for kind, *_ in ops) else umem
    A, Ln = descs["addr"].astype(np.int64), descs["len"].astype(np.int64)
    r0 = np.zeros(len(A), dtype=np.uint64)
    live = np.ones(len(A), dtype=bool)
    for kind, off, size, x in ops:
        if kind == "ld":
            if x:
                live &= off + size <= Ln
            i = np.nonzero(live)[0]
            r0[i] = r0[i] * np.uint64(31) + _gather(mem, A[i] + off, size)
            continue
        i = np.nonzero(live)[0]
        assert (off >= 0) and (off + size <= Ln[i]).all(), "a store outside its packet"
        mask = np.uint64(M64 >> (64 - 8 * size))
        v = np.full(len(i), x & M64, dtype=np.uint64)
        if kind == "add":
            v = (_gather(mem, A[i] + off, size) + v) & mask
        _scatter(mem, A[i] + off, size, v & mask)
    return r0, mem


def probe(off: int, size: int) -> list[int]:
    a = Asm()
    a.ldx(4, 2, 1, 0).ldx(4, 3, 1, 4)
    a.mov64(4, src=2).add64(4, off + size).jmp(JGT, 4, "short", src=3)
    a.ldx(size, 0, 2, off).exit()
    a.label("short").mov64(0, -1).exit()
    return a.assemble()


def probe_twin(off, size, umem, descs):
    A, Ln = descs["addr"].astype(np.int64), descs["len"].astype(np.int64)
    want = np.full(len(A), M64, dtype=np.uint64)
    i = np.nonzero(off + size <= Ln)[0]
    want[i] = _gather(umem, A[i] + off, size)
    return want


def fields(lo: int, hi: int):
    """(off, size) inside [lo, hi), sorted by end offset: every width at the first and at the last byte,
    and widths 2, 4, 8 across every 4-byte boundary (centred on it; at a 16-byte boundary also from the
    byte before it)."""
    f = {(lo, 1), (hi - 1, 1)}
    for w in SIZES:
        if lo + w <= hi:
            f |= {(lo, w), (hi - w, w)}
    for b in range((lo // 4 + 1) * 4, hi, 4):
        for w in SIZES[1:]:
            for o in (b - w // 2,) + ((b - 1,) if b % 16 == 0 else ()):
                if lo <= o and o + w <= hi:
                    f.add((o, w))
    return sorted(f, key=lambda x: (x[0] + x[1], x[0]))


def fold_ops(lo: int, hi: int):
    return tuple(("ld", off, size, True) for off, size in fields(lo, hi))


def no_read_program() -> list[int]:
    """Reads no packet byte: R0 = 1 where the packet has at least one byte, else 0."""
    a = Asm()
    a.ldx(4, 2, 1, 0).ldx(4, 3, 1, 4).mov64(0, 0)
    a.mov64(4, src=2).add64(4, 1).jmp(JGT, 4, "out", src=3).mov64(0, 1)
    a.label("out").exit()
    return a.assemble()


# ---------------------------------------------------------------- running and checking
_oracle_runs: dict = {}


def _oracle(oracle, key, prog, maps, umem, descs, entries):
    """The oracle's run of `prog` on a batch, computed once per (program, batch) and left unchanged."""
    k = (key, tuple(prog))
    if k not in _oracle_runs:
        _oracle_runs[k] = run_one(oracle, prog, maps, umem, descs, entries=entries)
    return _oracle_runs[k]


def check(lib, oracle, what, prog, want_r0, want_mem, batch_key, umem, descs, settings=None, maps=(), entries=None):
    """Run `prog` on `lib`; R0 and the UMEM bytes against numpy, then everything against the oracle."""
    settings = settings or Settings()
    a = run_one(lib, prog, list(maps), umem, descs, settings=settings, entries=entries)
    r = a[0]
    if settings.engine:
        assert r.stats["engine_used"] == settings.engine, f"{what}: engine {r.stats['engine_used']}"
    if settings.mode:
        assert r.stats["mode_used"] == settings.mode, f"{what}: mode {r.stats['mode_used']}"
    assert (r.results["status"] == 0).all(), f"{what}: status {np.unique(r.results['status'])}"
    got = r.results["r0"].view(np.uint64)
    bad = np.nonzero(got != want_r0)[0]
    assert not len(bad), (f"{what}: R0 of packet {bad[0]} (addr {descs['addr'][bad[0]]}, len {descs['len'][bad[0]]}) is "
                          f"{got[bad[0]]:#x}, numpy says {want_r0[bad[0]]:#x} ({len(bad)} of {len(got)} packets differ)")
    assert np.array_equal(a[2], want_mem), f"{what}: UMEM bytes differ from numpy"
    if oracle is not None:
        assert_same(a, _oracle(oracle, batch_key, prog, list(maps), umem, descs, entries), what)
    return r


def check_ops(lib, oracle, what, ops, batch_key, umem, descs, settings=None):
    want, mem = twin(ops, umem, descs)
    return check(lib, oracle, what, asm_ops(ops), want, mem, batch_key, umem, descs, settings)


def _settings(engine=0, mode=0):
    return Settings(engine=engine, mode=mode)


# 1 (and 5) ---- one load at every offset and width, window [0, 64)
def run_read_sweep(lib, oracle, size, tail_gap, engine=0, mode=0, seed=3):
    umem, descs = layout(seed, tail_gap)
    for off in PROBE_OFFS:
        check(lib, oracle, f"probe off {off} size {size} tail {tail_gap}", probe(off, size),
              probe_twin(off, size, umem, descs), umem, ("layout", seed, tail_gap), umem, descs, _settings(engine, mode))


# 2 (and 5) ---- per-program windows
def shape_window(lo, hi):
    """The (XE_HDR_LO, XE_HDR_HI) emit_window defines for a program reading [lo, hi): at most 49 bytes (four
    rows at any phase); none (the default [0, 64)) when the reads begin at byte 64 or above."""
    return None if lo >= 64 else (lo, min(hi, lo + 49))


def shape_programs():
    """name -> (program, ops or None): one fold per read range, and the program reading no packet byte."""
    progs = {f"{lo}_{hi}": (asm_ops(fold_ops(lo, hi)), fold_ops(lo, hi)) for lo, hi in SHAPES}
    progs["none"] = (no_read_program(), None)
    return progs


def _shape_want(ops, umem, descs):
    if ops is None:
        return (descs["len"] >= 1).astype(np.uint64), umem
    return twin(ops, umem, descs)


def run_window_shape(lib, oracle, name, tail_gap, engine=0, mode=0, seed=5):
    prog, ops = shape_programs()[name]
    umem, descs = layout(seed, tail_gap)
    want, mem = _shape_want(ops, umem, descs)
    check(lib, oracle, f"shape {name} tail {tail_gap}", prog, want, mem, ("layout", seed, tail_gap), umem, descs,
          _settings(engine, mode))


# 3 ---- three chunks and more per wave: both window buffers and their rotation
_many_want: dict = {}


def run_many_chunks(lib, shape, sched, engine=0, seed=7):
    import math
    ops = fold_ops(*shape)
    umem, descs = layout_many(seed)
    if shape not in _many_want:
        _many_want[shape] = twin(ops, umem, descs)[0]
        _many_want[shape].flags.writeable = False
    vm = VM(_settings(engine), lib=lib)
    try:
        vm.set_entrypoint(vm.add_raw_program(asm_ops(ops)))
        vm.set_schedule(sched)
        mem = umem.copy()
        r = vm.run_batch(mem, descs)
    finally:
        vm.close()
    if engine:
        assert r.stats["engine_used"] == engine
    assert r.stats["mode_used"] == MODE_PARALLEL
    # a wave must walk at least three chunks of 64 packets (4 waves a block), or the second buffer and the
    # rotation back to the first are not exercised
    chunks = math.ceil(len(descs) / 64)
    assert chunks >= 3 * 4 * r.stats["grid_blocks"], (chunks, r.stats["grid_blocks"])
    assert (r.results["status"] == 0).all()
    got = r.results["r0"].view(np.uint64)
    bad = np.nonzero(got != _many_want[shape])[0]
    assert not len(bad), f"shape {shape} schedule {sched}: {len(bad)} packets differ, first {bad[0]}"
    assert np.array_equal(mem, umem)


# 4 ---- windows at the end of the UMEM
def run_umem_tail(lib, oracle, shape, engine=0, mode=0):
    ops = fold_ops(*shape)
    for e in range(16):
        umem, descs = layout_tail(e, *shape)
        assert len(umem) % 16 == e and len(descs) == 65 + 16
        check_ops(lib, oracle, f"tail {e} shape {shape}", ops, ("tail", e, shape), umem, descs, _settings(engine, mode))


# 6 ---- stores across an edge of the window, then loads of the stored bytes
KINDS = {"st": (2, 4, 8), "stx": (2, 4, 8), "add": (4, 8)}


def _value(kind, size, n):
    """A store's operand: different for every store of a program, and its bytes differ from one another."""
    v = (0x1122334455667788 + 0x0101010101010101 * (n % 64)) & M64
    if kind == "st":
        v &= 0x7FFFFFFF  # ST's immediate
    return v


def _loads_after(off, size, lo, hi, limit):
    """A byte load at every byte of the store, and a load of the store's width at off - 1, off, off + 1;
    only loads inside [lo, hi) when the program's window must keep that shape, and below `limit`."""
    ld = [(off + b, 1) for b in range(size)] + [(off + d, size) for d in (-1, 0, 1)]
    return [("ld", o, s, False) for o, s in ld if lo <= o and o + s <= min(hi, limit)]


def edge_offsets(size, edge):
    """Offsets of a `size`-byte store with bytes on both sides of `edge`."""
    return range(edge - size + 1, edge)


def interp_store_offsets(size):
    """Window [0, 64): a packet at phase p has [0, 64 - p) in the window, so over the 16 phases the end
    lies at 49..64: every offset at which a store overlaps one of these ends."""
    return sorted({o for p in range(16) for o in edge_offsets(size, 64 - p)})


def write_ops(kind, size, off, length=100):
    return (("ld", 0, 1, False), (kind, off, size, _value(kind, size, off))) + tuple(_loads_after(off, size, 0, length, length))


def run_write_through(lib, oracle, kind, size, engine=0, mode=0, seed=11):
    umem, descs = layout_flat(seed)
    for off in interp_store_offsets(size):
        check_ops(lib, oracle, f"{kind}{size * 8} at {off}", write_ops(kind, size, off), ("flat", seed), umem, descs,
                  _settings(engine, mode))


# per-program kernels: ST / STX across the edges of a window shaped by the program's own reads. An atomic
# counts as a read in packet_read_range, so it always lies inside its kernel's [lo, hi); it reaches the end
# of the window only where the window is cut to four rows: a program reading byte 0 and adding across
# byte 49..64, where such a window ends at one of the 16 phases.
WRITE_SHAPES = ((12, 28), (16, 32))


def shaped_write_ops(kind, size, lo, hi):
    ops = [("ld", lo, 1, False), ("ld", hi - 1, 1, False)]  # the reads that give the window its shape
    for edge in (lo, hi):
        for off in edge_offsets(size, edge):
            ops.append((kind, off, size, _value(kind, size, len(ops))))
            ops += _loads_after(off, size, lo, hi, 100)
    return tuple(ops)


def capped_add_offsets(size):
    """Offsets size - 1 apart, so that every end 49..64 of the window has an add across it (an unaligned
    atomic add is a long piece of kernel: every offset of interp_store_offsets would compile for minutes)."""
    return range(49 - size + 1, 64, size - 1)


def capped_add_ops(size):
    ops = [("ld", 0, 1, False)]
    for off in capped_add_offsets(size):
        ops.append(("add", off, size, _value("add", size, len(ops))))
        ops += _loads_after(off, size, 0, 100, 100)
    return tuple(ops)


def jit_write_programs():
    progs = {f"{kind}{size}_{lo}_{hi}": shaped_write_ops(kind, size, lo, hi)
             for lo, hi in WRITE_SHAPES for kind in ("st", "stx") for size in KINDS[kind]}
    progs.update({f"add{size}_capped": capped_add_ops(size) for size in KINDS["add"]})
    return progs


def run_write_through_jit(lib, oracle, name, mode=0, seed=13):
    umem, descs = layout_flat(seed)
    check_ops(lib, oracle, f"jit write {name}", jit_write_programs()[name], ("flat", seed), umem, descs,
              _settings(ENGINE_JIT, mode))


# keyed: a 4-byte key stored across the end of the window, then looked up through the packet pointer
KEY, KEY_VALUE = 0x5AC3_71E9, 0x0123_4567_89AB_CDEF
KEY_MAP = (MapDef(MAP_HASH, 4, 8, 16), None)
KEY_ENTRIES = {0: [(KEY.to_bytes(4, "little"), KEY_VALUE.to_bytes(8, "little"))]}
JIT_KEY_OFFS = (58, 61)  # with the read of byte 0 the window is [0, 64 - phase): across its end at phases 3..5 / 0..2


def key_program(off: int) -> list[int]:
    a = Asm()
    a.ldx(4, 6, 1, 0).ldx(1, 7, 6, 0)  # r6 = data; the read of byte 0 keeps the window at [0, ...)
    a.st(4, 6, off, KEY)
    a.ld_map(1, 1).mov64(2, src=6).add64(2, off).call(1)
    a.jmp(JEQ, 0, "miss", imm=0)
    a.ldx(8, 0, 0, 0).exit()
    a.label("miss").mov64(0, -1).exit()
    return a.assemble()


def run_keyed(lib, oracle, offs, engine=0, mode=0, seed=17):
    umem, descs = layout_flat(seed)
    A = descs["addr"].astype(np.int64)
    for off in offs:
        mem = umem.copy()
        _scatter(mem, A + off, 4, np.full(len(A), KEY, dtype=np.uint64))
        want = np.full(len(A), KEY_VALUE, dtype=np.uint64)  # found (R0 not null) and the value loaded
        check(lib, oracle, f"key at {off}", key_program(off), want, mem, ("flat", seed), umem, descs,
              _settings(engine, mode), maps=[KEY_MAP], entries=KEY_ENTRIES)


MODES = (MODE_PARALLEL, MODE_SEQUENTIAL)
MODE_IDS = ("parallel", "sequential")


def kernel_cases():
    """The per-program kernels of these cases, for the ahead-of-time build (tests/kernel_cases.py)."""
    jit = Settings(engine=ENGINE_JIT)
    cases = [(prog, [], None, jit) for prog, _ in shape_programs().values()]
    cases.append((asm_ops(fold_ops(*FULL)), [], None, jit))  # the many-chunks and UMEM-tail batches
    cases += [(asm_ops(ops), [], None, jit) for ops in jit_write_programs().values()]
    cases += [(key_program(off), [KEY_MAP], KEY_ENTRIES, jit) for off in JIT_KEY_OFFS]
    return cases
