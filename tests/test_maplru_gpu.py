"""Device-side LRU_HASH lookup, delete, order and evict on the product library (gfx950 kernels,
gobpfld_amd/csrc/xe_mapops.hip): the cases of tests/maplru_cases.py with the keys and the outputs in device memory.
Here TOUCH's 64-bit atomic max decides among the repetitions of a key, CLAIM's CAS among the deleters of one, the
grouped probes read LRU records, the waves stride over the tiles of the stamp selection and the device radix sort
puts the selected slots in rank order."""
import numpy as np
import pytest
import torch

import maplru_cases as LC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("ks,vs,max_entries", LC.GEOMETRY)
def test_geometry(gpu_lib, oracle_lib, ks, vs, max_entries):
    LC.run_geometry(gpu_lib, oracle_lib, dev, ks, vs, max_entries)


@pytest.mark.parametrize("live", LC.LIVE_EDGES)
def test_live_entries_at_the_tile_edges(gpu_lib, oracle_lib, live):
    LC.run_live_edge(gpu_lib, oracle_lib, dev, live)


def test_lookup(gpu_lib, oracle_lib):
    LC.run_lookup(gpu_lib, oracle_lib, dev)


def test_device_calls_in_a_row(gpu_lib, oracle_lib):
    LC.run_chained(gpu_lib, oracle_lib, dev)


def test_peek_changes_nothing(gpu_lib, oracle_lib):
    LC.run_peek(gpu_lib, oracle_lib, dev)


def test_delete(gpu_lib, oracle_lib):
    LC.run_delete(gpu_lib, oracle_lib, dev)


def test_delete_then_a_batch_inserts_again(gpu_lib, oracle_lib):
    LC.run_delete_then_learn(gpu_lib, oracle_lib, dev)


def test_order(gpu_lib, oracle_lib):
    LC.run_order(gpu_lib, oracle_lib, dev)


def test_evict(gpu_lib, oracle_lib):
    LC.run_order(gpu_lib, oracle_lib, dev, evict=True)


def test_nil_backed_values(gpu_lib, oracle_lib):
    LC.run_nil_backed(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("mode", (0, LC.MODE_SEQUENTIAL), ids=("auto", "seq"))
def test_evict_then_a_learning_batch(gpu_lib, oracle_lib, mode):
    LC.run_evict_then_learn(gpu_lib, oracle_lib, dev, mode)


@pytest.mark.parametrize("state", LC.STATES)
def test_state_the_kernels_did_not_create(gpu_lib, oracle_lib, state):
    LC.run_state(gpu_lib, oracle_lib, dev, state)


def test_errors(gpu_lib):
    LC.run_errors(gpu_lib, dev)


@pytest.mark.parametrize("on_device", (False, True))
def test_python_interface(gpu_lib, oracle_lib, on_device):
    LC.run_python_api(gpu_lib, oracle_lib, dev, on_device)
