"""Batched device map lookup / update / delete on the product library (gfx950 kernels,
gobpfld_amd/csrc/xe_mapops.hip): the cases of tests/mapops_cases.py with keys and values in device
memory (CUDA tensors, passed through to the device entry points) and, for the matrix, also in host
memory (numpy arrays, staged by the host-pointer forms)."""
import numpy as np
import pytest
import torch

import mapops_cases as MC
from gobpfld_amd.emulator import MAP_ARRAY, MAP_HASH

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def staged(a):
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("vs", MC.VALUE_SIZES)
@pytest.mark.parametrize("ks", MC.KEY_SIZES)
def test_hash_matrix(gpu_lib, oracle_lib, ks, vs):
    # device tensors for half of the matrix, the host-pointer forms for the other half
    MC.run_matrix(gpu_lib, oracle_lib, dev if (MC.KEY_SIZES.index(ks) + MC.VALUE_SIZES.index(vs)) % 2 == 0 else staged,
                  MAP_HASH, ks, vs)


@pytest.mark.parametrize("vs", MC.VALUE_SIZES)
def test_array_matrix(gpu_lib, oracle_lib, vs):
    MC.run_matrix(gpu_lib, oracle_lib, dev if vs in (1, 24) else staged, MAP_ARRAY, 4, vs)


@pytest.mark.parametrize("ks,vs", MC.EDGE_PAIRS)
def test_hash_matrix_edges(gpu_lib, oracle_lib, ks, vs):
    MC.run_matrix(gpu_lib, oracle_lib, dev if MC.EDGE_PAIRS.index((ks, vs)) % 2 == 0 else staged, MAP_HASH, ks, vs,
                  counts=MC.EDGE_COUNTS)


@pytest.mark.parametrize("vs", MC.EDGE_VALUE_SIZES)
def test_array_matrix_edges(gpu_lib, oracle_lib, vs):
    MC.run_matrix(gpu_lib, oracle_lib, staged if MC.EDGE_VALUE_SIZES.index(vs) % 2 == 0 else dev, MAP_ARRAY, 4, vs,
                  counts=MC.EDGE_COUNTS)


@pytest.mark.parametrize("ks,vs", MC.ALIGN_HASH)
def test_hash_alignment(gpu_lib, oracle_lib, ks, vs):
    MC.run_alignment(gpu_lib, oracle_lib, dev, MAP_HASH, ks, vs)


@pytest.mark.parametrize("vs", MC.ALIGN_ARRAY)
def test_array_alignment(gpu_lib, oracle_lib, vs):
    MC.run_alignment(gpu_lib, oracle_lib, dev, MAP_ARRAY, 4, vs)


def test_contention(gpu_lib, oracle_lib):
    MC.run_contention(gpu_lib, oracle_lib, dev)


def test_nil_backed_values(gpu_lib, oracle_lib):
    MC.run_vlen0(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("ks", (8, 13, 24, 64))
def test_probe_chains(gpu_lib, oracle_lib, ks):
    MC.run_probe_chains(gpu_lib, oracle_lib, dev, ks=ks)


def test_duplicates(gpu_lib, oracle_lib):
    MC.run_duplicates(gpu_lib, oracle_lib, dev)


def test_tombstone_churn(gpu_lib, oracle_lib):
    MC.run_tombstone_churn(gpu_lib, oracle_lib, dev)


def test_limits(gpu_lib, oracle_lib):
    MC.run_limits(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_mixed_with_runs_and_host_path(gpu_lib, oracle_lib, use_async):
    MC.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_no_whole_map_traffic(gpu_lib):
    MC.run_traffic(gpu_lib, dev)


def test_epoch(gpu_lib):
    MC.run_epoch(gpu_lib, dev)
