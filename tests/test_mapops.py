"""Batched device map lookup / update / delete on the host simulation: the kernels' per-key decisions
(gobpfld_amd/csrc/xe_mapops.h) run as loops over host memory, against the oracle's single-key calls
(tests/mapops_cases.py). The product library runs the same cases in tests/test_mapops_gpu.py."""
import numpy as np
import pytest

import mapops_cases as MC
from gobpfld_amd.emulator import MAP_ARRAY, MAP_HASH


def dev(a):
    return np.ascontiguousarray(a)


def test_hash_restatement_guard(hostsim_lib):
    for ks in MC.GUARD_KEY_SIZES:
        MC.guard_hash_restatement(hostsim_lib, ks)


@pytest.mark.parametrize("vs", MC.VALUE_SIZES)
@pytest.mark.parametrize("ks", MC.KEY_SIZES)
def test_hash_matrix(hostsim_lib, oracle_lib, ks, vs):
    MC.run_matrix(hostsim_lib, oracle_lib, dev, MAP_HASH, ks, vs)


@pytest.mark.parametrize("vs", MC.VALUE_SIZES)
def test_array_matrix(hostsim_lib, oracle_lib, vs):
    MC.run_matrix(hostsim_lib, oracle_lib, dev, MAP_ARRAY, 4, vs)


@pytest.mark.parametrize("ks,vs", MC.EDGE_PAIRS)
def test_hash_matrix_edges(hostsim_lib, oracle_lib, ks, vs):
    MC.run_matrix(hostsim_lib, oracle_lib, dev, MAP_HASH, ks, vs, counts=MC.EDGE_COUNTS)


@pytest.mark.parametrize("vs", MC.EDGE_VALUE_SIZES)
def test_array_matrix_edges(hostsim_lib, oracle_lib, vs):
    MC.run_matrix(hostsim_lib, oracle_lib, dev, MAP_ARRAY, 4, vs, counts=MC.EDGE_COUNTS)


@pytest.mark.parametrize("ks,vs", MC.ALIGN_HASH)
def test_hash_alignment(hostsim_lib, oracle_lib, ks, vs):
    MC.run_alignment(hostsim_lib, oracle_lib, dev, MAP_HASH, ks, vs)


@pytest.mark.parametrize("vs", MC.ALIGN_ARRAY)
def test_array_alignment(hostsim_lib, oracle_lib, vs):
    MC.run_alignment(hostsim_lib, oracle_lib, dev, MAP_ARRAY, 4, vs)


def test_contention(hostsim_lib, oracle_lib):
    MC.run_contention(hostsim_lib, oracle_lib, dev)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    MC.run_vlen0(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("ks", (8, 13, 24, 64))
def test_probe_chains(hostsim_lib, oracle_lib, ks):
    MC.run_probe_chains(hostsim_lib, oracle_lib, dev, ks=ks)


def test_duplicates(hostsim_lib, oracle_lib):
    MC.run_duplicates(hostsim_lib, oracle_lib, dev)


def test_tombstone_churn(hostsim_lib, oracle_lib):
    MC.run_tombstone_churn(hostsim_lib, oracle_lib, dev)


def test_limits(hostsim_lib, oracle_lib):
    MC.run_limits(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_mixed_with_runs_and_host_path(hostsim_lib, oracle_lib, use_async):
    MC.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_no_whole_map_traffic(hostsim_lib):
    MC.run_traffic(hostsim_lib, dev)


def test_epoch(hostsim_lib):
    MC.run_epoch(hostsim_lib, dev)
