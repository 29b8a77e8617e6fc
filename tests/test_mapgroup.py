"""Device-side group-by on the host simulation: the per-slot decisions of the kernels
(gobpfld_amd/csrc/xe_mapops.h: GROUP_LOCATE, UNDO, PUBLISH, ADD after the scan's SELECT and SCAN) run as loops
over host memory, against a Python dict over the oracle's entries folded into an oracle VM
(tests/mapgroup_cases.py). The simulation runs one slot after another, so the claim races and the wave
combining exist on the device only (tests/test_mapgroup_gpu.py); it still pins down what the right answer is."""
import numpy as np
import pytest

import mapgroup_cases as GC


def dev(a):
    return np.ascontiguousarray(a)


def test_group_restatement():
    GC.check_group_table()


@pytest.mark.parametrize("live", GC.EDGE_COUNTS)
def test_tile_and_round_edges(hostsim_lib, oracle_lib, live):
    GC.run_edges(hostsim_lib, oracle_lib, dev, live)


def test_striding_waves(hostsim_lib, oracle_lib):
    GC.run_striding(hostsim_lib, oracle_lib, dev)


def test_one_hot_group(hostsim_lib, oracle_lib):
    GC.run_hot(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("ngroups", GC.FEW_GROUPS + (0,))
def test_few_groups(hostsim_lib, oracle_lib, ngroups):
    GC.run_few(hostsim_lib, oracle_lib, dev, ngroups)


def test_claims_on_a_wrapping_chain(hostsim_lib, oracle_lib):
    GC.run_chain(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("room", (GC.FIT_GROUPS, GC.FIT_GROUPS - 1))
def test_exact_fit_and_no_room(hostsim_lib, oracle_lib, room):
    GC.run_fit(hostsim_lib, oracle_lib, dev, room)


def test_array_index_out_of_range(hostsim_lib, oracle_lib):
    GC.run_array_range(hostsim_lib, oracle_lib, dev)


def test_tombstone_reuse(hostsim_lib, oracle_lib):
    GC.run_tombstone_reuse(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("shape", GC.KEY_SHAPES)
def test_key_shapes(hostsim_lib, oracle_lib, shape):
    GC.run_key_shape(hostsim_lib, oracle_lib, dev, shape)


def test_array_sides(hostsim_lib, oracle_lib):
    GC.run_array_sides(hostsim_lib, oracle_lib, dev)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    GC.run_vlen0(hostsim_lib, oracle_lib, dev)


def test_filters(hostsim_lib, oracle_lib):
    GC.run_filters(hostsim_lib, oracle_lib, dev)


def test_accumulation(hostsim_lib, oracle_lib):
    GC.run_accumulation(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_beside_traffic(hostsim_lib, oracle_lib, use_async):
    GC.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_epoch(hostsim_lib):
    GC.run_epoch(hostsim_lib, dev)


def test_limits(hostsim_lib, oracle_lib):
    GC.run_limits(hostsim_lib, oracle_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    GC.run_python_api(hostsim_lib, oracle_lib, dev)
