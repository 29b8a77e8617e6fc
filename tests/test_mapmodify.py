"""In-place edits of map value fields on the host simulation: the per-slot decisions of the kernels
(gobpfld_amd/csrc/xe_mapops.h: MODIFY_TILE, MODIFY_EDIT, MODIFY_MARK, MODIFY_KEYED) run as loops over host
memory, against a model of the ops over Python integers, a twin VM that gets scan, edit and update, and the
oracle (tests/mapmodify_cases.py). The product library runs the same cases in tests/test_mapmodify_gpu.py."""
import numpy as np
import pytest

import mapmodify_cases as MM
from gobpfld_amd.emulator import MAP_ARRAY, MAP_HASH


def dev(a):
    return np.ascontiguousarray(a)


def test_vector_table():
    MM.check_vector_table()


def test_vectors(hostsim_lib):
    MM.run_vectors(hostsim_lib, dev)


@pytest.mark.parametrize("ks,vs", MM.MATRIX_PAIRS)
def test_hash_matrix(hostsim_lib, oracle_lib, ks, vs):
    MM.run_hash_matrix(hostsim_lib, oracle_lib, dev, ks, vs, host_form=MM.MATRIX_PAIRS.index((ks, vs)) % 2 == 1)


@pytest.mark.parametrize("entries", MM.ARRAY_ENTRIES)
@pytest.mark.parametrize("vs", MM.ARRAY_VALUE_SIZES)
def test_array_matrix(hostsim_lib, oracle_lib, vs, entries):
    MM.run_array_matrix(hostsim_lib, oracle_lib, dev, vs, entries, host_form=vs in (24, 1025))


def test_array_tile_plus_one(hostsim_lib, oracle_lib):
    MM.run_array_tile_plus_one(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("max_entries,slots,live", MM.SLOT_CASES)
def test_slot_counts(hostsim_lib, oracle_lib, max_entries, slots, live):
    MM.run_slot_counts(hostsim_lib, oracle_lib, dev, max_entries, slots, live)


@pytest.mark.parametrize("vs", (13, 100))
def test_fields(hostsim_lib, oracle_lib, vs):
    MM.run_fields(hostsim_lib, oracle_lib, dev, vs, host_form=vs == 100)


@pytest.mark.parametrize("host_form", (False, True))
def test_edit_lists(hostsim_lib, oracle_lib, host_form):
    MM.run_edit_lists(hostsim_lib, oracle_lib, dev, 24 if not host_form else 70, host_form)


def test_token_bucket(hostsim_lib, oracle_lib):
    MM.run_token_bucket(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("report", (False, True))
def test_cap_entries(hostsim_lib, oracle_lib, report):
    MM.run_caps(hostsim_lib, oracle_lib, dev, report, host_form=report)


@pytest.mark.parametrize("host_form", (False, True))
def test_empty_key(hostsim_lib, oracle_lib, host_form):
    MM.run_empty_key(hostsim_lib, oracle_lib, dev, 24, host_form)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    MM.run_vlen0(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("vs", (8, 24, 65, 1025))
def test_nil_backed_value_sizes(hostsim_lib, oracle_lib, vs):
    MM.run_vlen0_sizes(hostsim_lib, oracle_lib, dev, vs)


@pytest.mark.parametrize("vs", MM.KEYED_VALUE_SIZES)
@pytest.mark.parametrize("kind", (MAP_HASH, MAP_ARRAY))
def test_keyed(hostsim_lib, oracle_lib, kind, vs):
    MM.run_keyed(hostsim_lib, oracle_lib, dev, kind, vs, host_form=vs in (24, 1025))


@pytest.mark.parametrize("count", MM.KEYED_COUNTS)
def test_keyed_counts(hostsim_lib, oracle_lib, count):
    MM.run_keyed_counts(hostsim_lib, oracle_lib, dev, count, host_form=count == 257)


@pytest.mark.parametrize("use_async", (False, True))
def test_under_traffic(hostsim_lib, oracle_lib, use_async):
    MM.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_epoch(hostsim_lib):
    MM.run_epoch(hostsim_lib, dev)


def test_limits(hostsim_lib, oracle_lib):
    MM.run_limits(hostsim_lib, oracle_lib, dev)


def test_determinism(hostsim_lib):
    MM.run_determinism(hostsim_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    MM.run_python_api(hostsim_lib, oracle_lib, dev, on_device=False)
