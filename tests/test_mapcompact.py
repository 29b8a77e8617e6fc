"""Device-side tombstone compaction on the host simulation: the per-slot and per-run decisions of the kernels
(gobpfld_amd/csrc/xe_mapops.h: COMPACT_MARK, the scan's SCAN, COMPACT_REBUILD) run as loops over host memory,
against a Python restatement of the call's definition over the image exported before it
(tests/mapcompact_cases.py). The simulation walks one run after another on one thread, so the lane-alone and
wave paths and the runs rebuilt side by side exist on the device only (tests/test_mapcompact_gpu.py); it still
pins down what the right answer is."""
import numpy as np
import pytest

import mapcompact_cases as CC


def dev(a):
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("vs", CC.VALUE_SIZES)
@pytest.mark.parametrize("ks", CC.KEY_SIZES)
def test_matrix(hostsim_lib, oracle_lib, ks, vs):
    CC.run_matrix(hostsim_lib, oracle_lib, dev, ks, vs)


@pytest.mark.parametrize("vs", (8, 24))
@pytest.mark.parametrize("which", CC.GEOMETRY)
@pytest.mark.parametrize("max_entries", CC.GEOMETRY_TABLES)
def test_geometry(hostsim_lib, oracle_lib, max_entries, which, vs):
    CC.run_geometry(hostsim_lib, oracle_lib, dev, max_entries, which, vs)


def test_only_tombstones(hostsim_lib, oracle_lib):
    CC.run_only_tombstones(hostsim_lib, oracle_lib, dev)


def test_no_tombstones(hostsim_lib, oracle_lib):
    CC.run_no_tombstones(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("slots", (CC.MAX_RUN, CC.MAX_RUN + 1))
def test_long_run(hostsim_lib, oracle_lib, slots):
    CC.run_long(hostsim_lib, oracle_lib, dev, slots)


def test_long_run_of_wide_values(hostsim_lib, oracle_lib):
    CC.run_long(hostsim_lib, oracle_lib, dev, CC.MAX_RUN, vs=24)


def test_no_free_record(hostsim_lib, oracle_lib):
    CC.run_no_free_record(hostsim_lib, oracle_lib, dev)


def test_flags_and_kinds(hostsim_lib, oracle_lib):
    CC.run_flags_and_kinds(hostsim_lib, oracle_lib, dev)


def test_nil_backed_records_move(hostsim_lib, oracle_lib):
    CC.run_vlen0(hostsim_lib, oracle_lib, dev)


def test_empty_key(hostsim_lib, oracle_lib):
    CC.run_empty_key(hostsim_lib, oracle_lib, dev)


def test_delta_base(hostsim_lib, oracle_lib):
    CC.run_delta_base(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_under_traffic(hostsim_lib, oracle_lib, use_async):
    CC.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_determinism(hostsim_lib, oracle_lib):
    CC.run_determinism(hostsim_lib, oracle_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    CC.run_python_api(hostsim_lib, oracle_lib, dev)
