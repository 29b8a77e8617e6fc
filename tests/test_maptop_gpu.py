"""Device-side top-K, evict and value statistics on the product library (gfx950 kernels,
gobpfld_amd/csrc/xe_mapops.hip): the cases of tests/maptop_cases.py with the outputs in device memory
(CUDA tensors, passed through to the device entry points) and, for part of the matrix, in host memory
(the host-pointer forms, staged through the VM's buffers)."""
import numpy as np
import pytest
import torch

import mapscan_cases as SC
import maptop_cases as TC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("host_form", (False, True))
def test_ties_hash(gpu_lib, oracle_lib, host_form):
    TC.run_ties_hash(gpu_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("host_form", (False, True))
def test_ties_array(gpu_lib, oracle_lib, host_form):
    TC.run_ties_array(gpu_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("byte", (0, 3, 7))
def test_digit_order(gpu_lib, oracle_lib, byte):
    TC.run_digits(gpu_lib, oracle_lib, dev, byte, host_form=byte == 3)


def test_one_bin(gpu_lib, oracle_lib):
    TC.run_one_bin(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("vs", TC.WIDTH_VALUE_SIZES)
def test_widths_and_offsets(gpu_lib, oracle_lib, vs):
    TC.run_widths(gpu_lib, oracle_lib, dev, vs, host_form=vs in (17, 1025))


@pytest.mark.parametrize("host_form", (False, True))
def test_filters(gpu_lib, oracle_lib, host_form):
    TC.run_filters(gpu_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("ks,vs", TC.SHAPE_PAIRS)
def test_shapes(gpu_lib, oracle_lib, ks, vs):
    TC.run_shape(gpu_lib, oracle_lib, dev, ks, vs, host_form=TC.SHAPE_PAIRS.index((ks, vs)) % 2 == 1)


def test_nil_backed_values(gpu_lib, oracle_lib):
    TC.run_vlen0(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("max_entries,slots,live", SC.SLOT_CASES)
def test_slot_counts(gpu_lib, oracle_lib, max_entries, slots, live):
    TC.run_slot_counts(gpu_lib, oracle_lib, dev, max_entries, slots, live)


def test_output_discipline(gpu_lib, oracle_lib):
    TC.run_output(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("host_form", (False, True))
def test_evict(gpu_lib, oracle_lib, host_form):
    TC.run_evict(gpu_lib, oracle_lib, dev, host_form)


def test_epoch(gpu_lib):
    TC.run_epoch(gpu_lib, dev)


def test_stats(gpu_lib, oracle_lib):
    TC.run_stats(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_beside_traffic(gpu_lib, oracle_lib, use_async):
    TC.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_no_whole_map_traffic(gpu_lib):
    TC.run_traffic(gpu_lib, dev)


def test_limits(gpu_lib, oracle_lib):
    TC.run_limits(gpu_lib, oracle_lib, dev)


def test_determinism(gpu_lib, oracle_lib):
    TC.run_determinism(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("on_device", (False, True))
def test_python_interface(gpu_lib, oracle_lib, on_device):
    TC.run_python_api(gpu_lib, oracle_lib, dev, on_device)
