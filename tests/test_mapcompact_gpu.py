"""Device-side tombstone compaction on the product library (gfx950 kernels, gobpfld_amd/csrc/xe_mapops.hip): the
cases of tests/mapcompact_cases.py with the maps' inputs in device memory. Here the runs of a table are rebuilt
side by side, small values by their run's lane and large ones by the whole wave."""
import numpy as np
import pytest
import torch

import mapcompact_cases as CC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("vs", CC.VALUE_SIZES)
@pytest.mark.parametrize("ks", CC.KEY_SIZES)
def test_matrix(gpu_lib, oracle_lib, ks, vs):
    CC.run_matrix(gpu_lib, oracle_lib, dev, ks, vs)


@pytest.mark.parametrize("vs", (8, 24))
@pytest.mark.parametrize("which", CC.GEOMETRY)
@pytest.mark.parametrize("max_entries", CC.GEOMETRY_TABLES)
def test_geometry(gpu_lib, oracle_lib, max_entries, which, vs):
    CC.run_geometry(gpu_lib, oracle_lib, dev, max_entries, which, vs)


def test_only_tombstones(gpu_lib, oracle_lib):
    CC.run_only_tombstones(gpu_lib, oracle_lib, dev)


def test_no_tombstones(gpu_lib, oracle_lib):
    CC.run_no_tombstones(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("slots", (CC.MAX_RUN, CC.MAX_RUN + 1))
def test_long_run(gpu_lib, oracle_lib, slots):
    CC.run_long(gpu_lib, oracle_lib, dev, slots)


def test_long_run_of_wide_values(gpu_lib, oracle_lib):
    CC.run_long(gpu_lib, oracle_lib, dev, CC.MAX_RUN, vs=24)


def test_no_free_record(gpu_lib, oracle_lib):
    CC.run_no_free_record(gpu_lib, oracle_lib, dev)


def test_flags_and_kinds(gpu_lib, oracle_lib):
    CC.run_flags_and_kinds(gpu_lib, oracle_lib, dev)


def test_nil_backed_records_move(gpu_lib, oracle_lib):
    CC.run_vlen0(gpu_lib, oracle_lib, dev)


def test_empty_key(gpu_lib, oracle_lib):
    CC.run_empty_key(gpu_lib, oracle_lib, dev)


def test_delta_base(gpu_lib, oracle_lib):
    CC.run_delta_base(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_under_traffic(gpu_lib, oracle_lib, use_async):
    CC.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_determinism(gpu_lib, oracle_lib):
    CC.run_determinism(gpu_lib, oracle_lib, dev)


def test_python_interface(gpu_lib, oracle_lib):
    CC.run_python_api(gpu_lib, oracle_lib, dev)
