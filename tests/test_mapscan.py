"""Device-side map scan and expire on the host simulation: the per-slot decisions of the kernels
(gobpfld_amd/csrc/xe_mapops.h: SELECT, SCAN, SCATTER, COPY, EXPIRE) run as loops over host memory,
against the oracle's dump filtered by a numpy restatement of the filter (tests/mapscan_cases.py). The
product library runs the same cases in tests/test_mapscan_gpu.py."""
import numpy as np
import pytest

import mapscan_cases as SC


def dev(a):
    return np.ascontiguousarray(a)


def test_predicate_restatement():
    SC.check_predicate_table()


@pytest.mark.parametrize("ks,vs", SC.MATRIX_PAIRS)
def test_hash_matrix(hostsim_lib, oracle_lib, ks, vs):
    SC.run_hash_matrix(hostsim_lib, oracle_lib, dev, ks, vs, host_form=SC.MATRIX_PAIRS.index((ks, vs)) % 2 == 1)


@pytest.mark.parametrize("entries", SC.ARRAY_ENTRIES)
@pytest.mark.parametrize("vs", SC.ARRAY_VALUE_SIZES)
def test_array_matrix(hostsim_lib, oracle_lib, vs, entries):
    SC.run_array_matrix(hostsim_lib, oracle_lib, dev, vs, entries, host_form=vs in (24, 1025))


@pytest.mark.parametrize("max_entries,slots,live", SC.SLOT_CASES)
def test_slot_counts(hostsim_lib, oracle_lib, max_entries, slots, live):
    SC.run_slot_counts(hostsim_lib, oracle_lib, dev, max_entries, slots, live)


def test_array_tile_plus_one(hostsim_lib, oracle_lib):
    SC.run_array_tile_plus_one(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("expire", (False, True))
def test_cap_entries(hostsim_lib, oracle_lib, expire):
    SC.run_caps(hostsim_lib, oracle_lib, dev, expire)


@pytest.mark.parametrize("host_form", (False, True))
def test_fields(hostsim_lib, oracle_lib, host_form):
    SC.run_fields(hostsim_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("host_form", (False, True))
def test_empty_key(hostsim_lib, oracle_lib, host_form):
    SC.run_empty_key(hostsim_lib, oracle_lib, dev, 24, host_form)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    SC.run_vlen0(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("ks,vs", SC.ALIGN_PAIRS)
def test_alignment(hostsim_lib, oracle_lib, ks, vs):
    SC.run_alignment(hostsim_lib, oracle_lib, dev, ks, vs)


def test_expire_then_reuse(hostsim_lib, oracle_lib):
    SC.run_expire_reuse(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_under_traffic(hostsim_lib, oracle_lib, use_async):
    SC.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_no_whole_map_traffic(hostsim_lib):
    SC.run_traffic(hostsim_lib, dev)


def test_epoch(hostsim_lib):
    SC.run_epoch(hostsim_lib, dev)


def test_limits(hostsim_lib, oracle_lib):
    SC.run_limits(hostsim_lib, oracle_lib, dev)


def test_determinism(hostsim_lib, oracle_lib):
    SC.run_determinism(hostsim_lib, oracle_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    SC.run_python_api(hostsim_lib, oracle_lib, dev, on_device=False)
