"""Verdict dispatch and TX gather on the device (gobpfld_amd/csrc/xe_dispatch.hip): the matrices of
test_dispatch.py on the product library, a batch with more tiles than the scan takes in one pass, and
two end-to-end runs (emulate, dispatch, gather) against the oracle put through the numpy reference."""
import numpy as np
import pytest

import dispatch_cases as DC
from gobpfld_amd import _native as N
from gobpfld_amd import workloads as W
from gobpfld_amd import xsk as X
from gobpfld_amd.asm import JGT, Asm
from gobpfld_amd.dispatch import Dispatcher
from gobpfld_amd.emulator import VM, Settings

pytestmark = pytest.mark.gpu

# the scan kernel takes 1024 threads x 16 counts of the 7-row count array per pass, the counts of 2340
# tiles: this batch needs a second pass
MANY_TILES = 2400 * DC.T + 3


@pytest.mark.parametrize("n", DC.SIZES)
def test_dispatch_equals_numpy(gpu_lib, n):
    DC.check_dispatch(gpu_lib, True, n)


def test_dispatch_scan_loops(gpu_lib):
    DC.check_dispatch(gpu_lib, True, MANY_TILES, names=("uniform", "failed10"))


@pytest.mark.parametrize("ver_offset", (1, 2, 3))
@pytest.mark.parametrize("n", DC.UNALIGNED_SIZES)
def test_dispatch_unaligned_verdicts(gpu_lib, n, ver_offset):
    DC.check_dispatch(gpu_lib, True, n, names=("uniform", "failed10"), ver_offset=ver_offset)


def test_dispatch_argument_errors(gpu_lib):
    DC.check_errors(gpu_lib, True)


@pytest.mark.parametrize("room", DC.STRIDE_ROOMS)
def test_gather_grid_stride(gpu_lib, room):
    DC.check_gather_stride(gpu_lib, True, room)


@pytest.mark.parametrize("room", DC.ROOMS)
def test_gather_matrix_and_bounds(gpu_lib, room):
    DC.check_gather(gpu_lib, True, room)


def _first_byte_program():
    """return data[0]; a packet without a first byte takes the load anyway and ends in a VM error."""
    a = Asm()
    a.ldx(4, 6, 1, 0)                      # r6 = ctx->data
    a.ldx(4, 7, 1, 4)                      # r7 = ctx->data_end
    a.mov64(2, src=6).add64(2, 1)
    a.jmp(JGT, 2, "short", src=7)          # if data + 1 > data_end
    a.ldx(1, 0, 6, 0).exit()
    a.label("short")
    a.ldx(1, 0, 6, 0).exit()               # out of bounds
    return a.assemble()


def test_emulate_dispatch_gather_equals_oracle(gpu_lib, oracle_lib):
    import torch
    n, slot = 4099, 128
    rng = np.random.default_rng(2)
    umem = rng.integers(0, 256, size=n * slot, dtype=np.uint8)
    desc = np.zeros(n, DC.DESC)
    i = np.arange(n)
    desc["addr"] = i * slot + i % 5
    desc["len"] = np.where(i % 512 == 100, 0, 1 + (i * 7) % 90)
    umem[desc["addr"]] = i % 7
    ref = VM(Settings(), lib=oracle_lib)
    ref.set_entrypoint(ref.add_raw_program(_first_byte_program()))
    want = ref.run_batch(umem.copy(), desc)
    ref.close()
    status = want.results["status"]
    assert (status != 0).sum() == (desc["len"] == 0).sum() > 0 and set(want.verdicts[status == 0]) == set(range(7))
    order, offset, invalid, failed = DC.reference(want.verdicts, status)

    vm = VM(Settings(engine=1), lib=gpu_lib)  # the shared interpreter kernel: nothing to compile
    vm.set_entrypoint(vm.add_raw_program(_first_byte_program()))
    d_umem, d_desc = torch.from_numpy(umem).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda()
    d_res = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    d_ver = torch.empty(n, dtype=torch.int32, device="cuda")
    vm.run_batch_device(d_umem.data_ptr(), d_umem.numel(), d_desc.data_ptr(), n, d_results=d_res.data_ptr(),
                        d_verdicts=d_ver.data_ptr())
    dsp = Dispatcher(gpu_lib)
    part = dsp.run(d_desc.data_ptr(), d_ver.data_ptr(), n, d_results=d_res.data_ptr())
    c = part.counts()
    assert (c.offset, c.invalid, c.failed) == (offset, invalid, failed)
    assert (part.index_host() == order).all() and (part.desc_host() == desc[order]).all()

    tx = np.flatnonzero((status == 0) & (want.verdicts == 3))
    assert len(tx) == c.sizes[N.ACT_TX] > 0
    d_frames = torch.from_numpy((np.arange(len(tx), dtype=np.int64) * slot)).cuda()
    d_dst = torch.full((len(tx) * slot,), 0xEE, dtype=torch.uint8, device="cuda")
    g = dsp.gather(d_umem.data_ptr(), d_umem.numel(), part, N.ACT_TX, d_frames.data_ptr(), slot, d_dst.data_ptr(),
                   d_dst.numel(), max_count=len(tx))
    expect = np.full(len(tx) * slot, 0xEE, np.uint8)
    for k, p in enumerate(tx):
        a, ln = int(desc["addr"][p]), int(desc["len"][p])
        expect[k * slot:k * slot + ln] = umem[a:a + ln]
    assert g.rejected() == 0
    out = g.desc_host()
    assert (out["addr"] == np.arange(len(tx)) * slot).all() and (out["len"] == desc["len"][tx]).all() and not out["options"].any()
    assert (d_dst.cpu().numpy() == expect).all()
    assert (d_umem.cpu().numpy() == umem).all()
    vm.close()


def test_run_pcap_dispatch_counts_equal_oracle(gpu_lib, oracle_lib, tmp_path):
    n = 4096
    umem, descs = W.build_batch("c2", 0, n)
    pk = [umem[int(d["addr"]):int(d["addr"]) + int(d["len"])].tobytes() for d in descs]
    path = tmp_path / "c2.pcap"
    X.write_pcap(path, pk)
    ref = VM(Settings(), lib=oracle_lib)
    W.setup_vm(ref, "c2")
    want = ref.run_batch(umem.copy(), descs)
    ref.close()
    _, offset, _, _ = DC.reference(want.verdicts, want.results["status"])
    vm = VM(Settings(), lib=gpu_lib)
    W.setup_vm(vm, "c2")
    pc = X.PcapFile(path)
    res = X.run_pcap(vm, pc, batch=1 << 11, keep_verdicts=True, dispatch=True)
    pc.rewind()
    lean = X.run_pcap(vm, pc, batch=1 << 11, dispatch=True)
    vm.close()
    pc.close()
    assert res.packets == n and res.batches == 2
    assert res.action_count == np.diff(offset).tolist()
    assert (res.verdicts == want.verdicts).all() and sum(res.verdict_count.values()) == n
    assert lean.action_count == res.action_count and lean.verdicts is None and lean.verdict_count == {}
