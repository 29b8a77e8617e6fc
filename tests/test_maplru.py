"""Device-side LRU_HASH lookup, delete, order and evict on the host simulation: the per-key and per-slot
decisions of the kernels (gobpfld_amd/csrc/xe_mapops.h: FIND, VALUE, TOUCH; CLAIM, ERASE; the top's selection over
the stamps, RANK, SORT, COPY) run as loops over host memory, against an oracle VM that gets the same keys one at a
time (tests/maplru_cases.py). The simulation runs one entry after another with the plain probe and a
std::stable_sort, so the atomic max of TOUCH, the CAS of CLAIM, the striding waves and the device radix sort exist
on the device only (tests/test_maplru_gpu.py); it still pins down what the right answer is."""
import numpy as np
import pytest

import maplru_cases as LC


def dev(a):
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("ks,vs,max_entries", LC.GEOMETRY)
def test_geometry(hostsim_lib, oracle_lib, ks, vs, max_entries):
    LC.run_geometry(hostsim_lib, oracle_lib, dev, ks, vs, max_entries)


@pytest.mark.parametrize("live", LC.LIVE_EDGES)
def test_live_entries_at_the_tile_edges(hostsim_lib, oracle_lib, live):
    LC.run_live_edge(hostsim_lib, oracle_lib, dev, live)


def test_lookup(hostsim_lib, oracle_lib):
    LC.run_lookup(hostsim_lib, oracle_lib, dev)


def test_device_calls_in_a_row(hostsim_lib, oracle_lib):
    LC.run_chained(hostsim_lib, oracle_lib, dev)


def test_peek_changes_nothing(hostsim_lib, oracle_lib):
    LC.run_peek(hostsim_lib, oracle_lib, dev)


def test_delete(hostsim_lib, oracle_lib):
    LC.run_delete(hostsim_lib, oracle_lib, dev)


def test_delete_then_a_batch_inserts_again(hostsim_lib, oracle_lib):
    LC.run_delete_then_learn(hostsim_lib, oracle_lib, dev)


def test_order(hostsim_lib, oracle_lib):
    LC.run_order(hostsim_lib, oracle_lib, dev)


def test_evict(hostsim_lib, oracle_lib):
    LC.run_order(hostsim_lib, oracle_lib, dev, evict=True)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    LC.run_nil_backed(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("mode", (0, LC.MODE_SEQUENTIAL), ids=("auto", "seq"))
def test_evict_then_a_learning_batch(hostsim_lib, oracle_lib, mode):
    LC.run_evict_then_learn(hostsim_lib, oracle_lib, dev, mode)


@pytest.mark.parametrize("state", LC.STATES)
def test_state_the_kernels_did_not_create(hostsim_lib, oracle_lib, state):
    LC.run_state(hostsim_lib, oracle_lib, dev, state)


def test_errors(hostsim_lib):
    LC.run_errors(hostsim_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    LC.run_python_api(hostsim_lib, oracle_lib, dev, False)
