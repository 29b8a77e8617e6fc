"""In-place edits of map value fields on the product library (gfx950 kernels,
gobpfld_amd/csrc/xe_mapops.hip): the cases of tests/mapmodify_cases.py with the keys and the outputs in device
memory (CUDA tensors, passed through to the device entry points) and, for part of every matrix, in host memory
(the host-pointer forms, staged through the VM's buffers)."""
import numpy as np
import pytest
import torch

import mapmodify_cases as MM
from gobpfld_amd.emulator import MAP_ARRAY, MAP_HASH

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_vectors(gpu_lib):
    MM.run_vectors(gpu_lib, dev)


@pytest.mark.parametrize("ks,vs", MM.MATRIX_PAIRS)
def test_hash_matrix(gpu_lib, oracle_lib, ks, vs):
    MM.run_hash_matrix(gpu_lib, oracle_lib, dev, ks, vs, host_form=MM.MATRIX_PAIRS.index((ks, vs)) % 2 == 1)


@pytest.mark.parametrize("entries", MM.ARRAY_ENTRIES)
@pytest.mark.parametrize("vs", MM.ARRAY_VALUE_SIZES)
def test_array_matrix(gpu_lib, oracle_lib, vs, entries):
    MM.run_array_matrix(gpu_lib, oracle_lib, dev, vs, entries, host_form=vs in (24, 1025))


def test_array_tile_plus_one(gpu_lib, oracle_lib):
    MM.run_array_tile_plus_one(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("max_entries,slots,live", MM.SLOT_CASES)
def test_slot_counts(gpu_lib, oracle_lib, max_entries, slots, live):
    MM.run_slot_counts(gpu_lib, oracle_lib, dev, max_entries, slots, live)


@pytest.mark.parametrize("vs", (13, 100))
def test_fields(gpu_lib, oracle_lib, vs):
    MM.run_fields(gpu_lib, oracle_lib, dev, vs, host_form=vs == 100)


@pytest.mark.parametrize("host_form", (False, True))
def test_edit_lists(gpu_lib, oracle_lib, host_form):
    MM.run_edit_lists(gpu_lib, oracle_lib, dev, 24 if not host_form else 70, host_form)


def test_token_bucket(gpu_lib, oracle_lib):
    MM.run_token_bucket(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("report", (False, True))
def test_cap_entries(gpu_lib, oracle_lib, report):
    MM.run_caps(gpu_lib, oracle_lib, dev, report, host_form=report)


@pytest.mark.parametrize("host_form", (False, True))
def test_empty_key(gpu_lib, oracle_lib, host_form):
    MM.run_empty_key(gpu_lib, oracle_lib, dev, 24, host_form)


def test_nil_backed_values(gpu_lib, oracle_lib):
    MM.run_vlen0(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("vs", (8, 24, 65, 1025))
def test_nil_backed_value_sizes(gpu_lib, oracle_lib, vs):
    MM.run_vlen0_sizes(gpu_lib, oracle_lib, dev, vs)


@pytest.mark.parametrize("vs", MM.KEYED_VALUE_SIZES)
@pytest.mark.parametrize("kind", (MAP_HASH, MAP_ARRAY))
def test_keyed(gpu_lib, oracle_lib, kind, vs):
    MM.run_keyed(gpu_lib, oracle_lib, dev, kind, vs, host_form=vs in (24, 1025))


@pytest.mark.parametrize("count", MM.KEYED_COUNTS)
def test_keyed_counts(gpu_lib, oracle_lib, count):
    MM.run_keyed_counts(gpu_lib, oracle_lib, dev, count, host_form=count == 257)


@pytest.mark.parametrize("use_async", (False, True))
def test_under_traffic(gpu_lib, oracle_lib, use_async):
    MM.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_epoch(gpu_lib):
    MM.run_epoch(gpu_lib, dev)


def test_limits(gpu_lib, oracle_lib):
    MM.run_limits(gpu_lib, oracle_lib, dev)


def test_determinism(gpu_lib):
    MM.run_determinism(gpu_lib, dev)


@pytest.mark.parametrize("on_device", (False, True))
def test_python_interface(gpu_lib, oracle_lib, on_device):
    MM.run_python_api(gpu_lib, oracle_lib, dev, on_device)
