"""Device-side group-by on the product library (gfx950 kernels, gobpfld_amd/csrc/xe_mapops.hip): the cases of
tests/mapgroup_cases.py with the maps' inputs in device memory. Here the claims of GROUP_LOCATE race, the waves
of GROUP_ADD combine, and the tile passes stride."""
import numpy as np
import pytest
import torch

import mapgroup_cases as GC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("live", GC.EDGE_COUNTS)
def test_tile_and_round_edges(gpu_lib, oracle_lib, live):
    GC.run_edges(gpu_lib, oracle_lib, dev, live)


def test_striding_waves(gpu_lib, oracle_lib):
    GC.run_striding(gpu_lib, oracle_lib, dev)


def test_one_hot_group(gpu_lib, oracle_lib):
    GC.run_hot(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("ngroups", GC.FEW_GROUPS + (0,))
def test_few_groups(gpu_lib, oracle_lib, ngroups):
    GC.run_few(gpu_lib, oracle_lib, dev, ngroups)


def test_claims_on_a_wrapping_chain(gpu_lib, oracle_lib):
    GC.run_chain(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("room", (GC.FIT_GROUPS, GC.FIT_GROUPS - 1))
def test_exact_fit_and_no_room(gpu_lib, oracle_lib, room):
    GC.run_fit(gpu_lib, oracle_lib, dev, room)


def test_array_index_out_of_range(gpu_lib, oracle_lib):
    GC.run_array_range(gpu_lib, oracle_lib, dev)


def test_tombstone_reuse(gpu_lib, oracle_lib):
    GC.run_tombstone_reuse(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("shape", GC.KEY_SHAPES)
def test_key_shapes(gpu_lib, oracle_lib, shape):
    GC.run_key_shape(gpu_lib, oracle_lib, dev, shape)


def test_array_sides(gpu_lib, oracle_lib):
    GC.run_array_sides(gpu_lib, oracle_lib, dev)


def test_nil_backed_values(gpu_lib, oracle_lib):
    GC.run_vlen0(gpu_lib, oracle_lib, dev)


def test_filters(gpu_lib, oracle_lib):
    GC.run_filters(gpu_lib, oracle_lib, dev)


def test_accumulation(gpu_lib, oracle_lib):
    GC.run_accumulation(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_beside_traffic(gpu_lib, oracle_lib, use_async):
    GC.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_epoch(gpu_lib):
    GC.run_epoch(gpu_lib, dev)


def test_limits(gpu_lib, oracle_lib):
    GC.run_limits(gpu_lib, oracle_lib, dev)


def test_python_interface(gpu_lib, oracle_lib):
    GC.run_python_api(gpu_lib, oracle_lib, dev)
