"""Device-side top-K, evict and value statistics on the host simulation: the per-slot decisions of the
kernels (gobpfld_amd/csrc/xe_mapops.h: PREFIX, PICK, CUT, TRIM, STATS and the scan's steps) run as loops
over host memory, against the oracle's entries ranked by a numpy restatement (tests/maptop_cases.py). The
product library runs the same cases in tests/test_maptop_gpu.py."""
import numpy as np
import pytest

import mapscan_cases as SC
import maptop_cases as TC


def dev(a):
    return np.ascontiguousarray(a)


def test_rank_restatement():
    TC.check_rank_table()


@pytest.mark.parametrize("host_form", (False, True))
def test_ties_hash(hostsim_lib, oracle_lib, host_form):
    TC.run_ties_hash(hostsim_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("host_form", (False, True))
def test_ties_array(hostsim_lib, oracle_lib, host_form):
    TC.run_ties_array(hostsim_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("byte", (0, 3, 7))
def test_digit_order(hostsim_lib, oracle_lib, byte):
    TC.run_digits(hostsim_lib, oracle_lib, dev, byte, host_form=byte == 3)


def test_one_bin(hostsim_lib, oracle_lib):
    TC.run_one_bin(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("vs", TC.WIDTH_VALUE_SIZES)
def test_widths_and_offsets(hostsim_lib, oracle_lib, vs):
    TC.run_widths(hostsim_lib, oracle_lib, dev, vs, host_form=vs in (17, 1025))


@pytest.mark.parametrize("host_form", (False, True))
def test_filters(hostsim_lib, oracle_lib, host_form):
    TC.run_filters(hostsim_lib, oracle_lib, dev, host_form)


@pytest.mark.parametrize("ks,vs", TC.SHAPE_PAIRS)
def test_shapes(hostsim_lib, oracle_lib, ks, vs):
    TC.run_shape(hostsim_lib, oracle_lib, dev, ks, vs, host_form=TC.SHAPE_PAIRS.index((ks, vs)) % 2 == 1)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    TC.run_vlen0(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("max_entries,slots,live", SC.SLOT_CASES)
def test_slot_counts(hostsim_lib, oracle_lib, max_entries, slots, live):
    TC.run_slot_counts(hostsim_lib, oracle_lib, dev, max_entries, slots, live)


def test_output_discipline(hostsim_lib, oracle_lib):
    TC.run_output(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("host_form", (False, True))
def test_evict(hostsim_lib, oracle_lib, host_form):
    TC.run_evict(hostsim_lib, oracle_lib, dev, host_form)


def test_epoch(hostsim_lib):
    TC.run_epoch(hostsim_lib, dev)


def test_stats(hostsim_lib, oracle_lib):
    TC.run_stats(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_beside_traffic(hostsim_lib, oracle_lib, use_async):
    TC.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_no_whole_map_traffic(hostsim_lib):
    TC.run_traffic(hostsim_lib, dev)


def test_limits(hostsim_lib, oracle_lib):
    TC.run_limits(hostsim_lib, oracle_lib, dev)


def test_determinism(hostsim_lib, oracle_lib):
    TC.run_determinism(hostsim_lib, oracle_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    TC.run_python_api(hostsim_lib, oracle_lib, dev, on_device=False)
