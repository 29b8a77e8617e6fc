"""Device-side map scan and expire on the product library (gfx950 kernels,
gobpfld_amd/csrc/xe_mapops.hip): the cases of tests/mapscan_cases.py with the outputs in device memory
(CUDA tensors, passed through to the device entry points) and, for part of the matrix, in host memory
(the host-pointer forms, staged through the VM's buffers)."""
import numpy as np
import pytest
import torch

import mapscan_cases as SC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("ks,vs", SC.MATRIX_PAIRS)
def test_hash_matrix(gpu_lib, oracle_lib, ks, vs):
    SC.run_hash_matrix(gpu_lib, oracle_lib, dev, ks, vs, host_form=SC.MATRIX_PAIRS.index((ks, vs)) % 2 == 1)


@pytest.mark.parametrize("entries", SC.ARRAY_ENTRIES)
@pytest.mark.parametrize("vs", SC.ARRAY_VALUE_SIZES)
def test_array_matrix(gpu_lib, oracle_lib, vs, entries):
    SC.run_array_matrix(gpu_lib, oracle_lib, dev, vs, entries, host_form=vs in (24, 1025))


@pytest.mark.parametrize("max_entries,slots,live", SC.SLOT_CASES)
def test_slot_counts(gpu_lib, oracle_lib, max_entries, slots, live):
    SC.run_slot_counts(gpu_lib, oracle_lib, dev, max_entries, slots, live)


def test_array_tile_plus_one(gpu_lib, oracle_lib):
    SC.run_array_tile_plus_one(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("expire", (False, True))
def test_cap_entries(gpu_lib, oracle_lib, expire):
    SC.run_caps(gpu_lib, oracle_lib, dev, expire)


@pytest.mark.parametrize("host_form", (False, True))
def test_fields(gpu_lib, oracle_lib, host_form):
    SC.run_fields(gpu_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("host_form", (False, True))
def test_empty_key(gpu_lib, oracle_lib, host_form):
    SC.run_empty_key(gpu_lib, oracle_lib, dev, 24, host_form)


def test_nil_backed_values(gpu_lib, oracle_lib):
    SC.run_vlen0(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("ks,vs", SC.ALIGN_PAIRS)
def test_alignment(gpu_lib, oracle_lib, ks, vs):
    SC.run_alignment(gpu_lib, oracle_lib, dev, ks, vs)


def test_expire_then_reuse(gpu_lib, oracle_lib):
    SC.run_expire_reuse(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_under_traffic(gpu_lib, oracle_lib, use_async):
    SC.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_no_whole_map_traffic(gpu_lib):
    SC.run_traffic(gpu_lib, dev)


def test_epoch(gpu_lib):
    SC.run_epoch(gpu_lib, dev)


def test_limits(gpu_lib, oracle_lib):
    SC.run_limits(gpu_lib, oracle_lib, dev)


def test_determinism(gpu_lib, oracle_lib):
    SC.run_determinism(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("on_device", (False, True))
def test_python_interface(gpu_lib, oracle_lib, on_device):
    SC.run_python_api(gpu_lib, oracle_lib, dev, on_device)
