"""Device-side join on the product library (gfx950 kernels, gobpfld_amd/csrc/xe_mapops.hip): the cases of
tests/mapjoin_cases.py with the maps' inputs and the outputs in device memory. Here the probes of JOIN_SELECT
diverge in front of its ballots, the grouped probes read the other map's records, the waves stride over the tiles
and JOIN_VALUE's sub-groups follow the other map's value size."""
import numpy as np
import pytest
import torch

import mapjoin_cases as JC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("mode", JC.MODES)
@pytest.mark.parametrize("live", JC.EDGE_COUNTS)
def test_tile_and_round_edges(gpu_lib, oracle_lib, live, mode):
    JC.run_edges(gpu_lib, oracle_lib, dev, live, mode)


def test_striding_waves(gpu_lib, oracle_lib):
    JC.run_striding(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("shape", JC.JOIN_SHAPES)
def test_probe_paths(gpu_lib, oracle_lib, shape):
    JC.run_shape(gpu_lib, oracle_lib, dev, shape)


@pytest.mark.parametrize("ks", JC.CHAIN_KEY_SIZES)
def test_chains_in_the_other_map(gpu_lib, oracle_lib, ks):
    JC.run_chains(gpu_lib, oracle_lib, dev, ks)


def test_nil_backed_values(gpu_lib, oracle_lib):
    JC.run_vlen0(gpu_lib, oracle_lib, dev)


def test_array_sides(gpu_lib, oracle_lib):
    JC.run_array_sides(gpu_lib, oracle_lib, dev)


def test_filters(gpu_lib, oracle_lib):
    JC.run_filters(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("host_form", (False, True))
def test_removal(gpu_lib, oracle_lib, host_form):
    JC.run_removal(gpu_lib, oracle_lib, dev, host_form)


def test_removal_writes_the_delta_base(gpu_lib):
    JC.run_removal_delta(gpu_lib, dev)


def test_self_join(gpu_lib, oracle_lib):
    JC.run_self_join(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_beside_traffic(gpu_lib, oracle_lib, use_async):
    JC.run_mixed(gpu_lib, oracle_lib, dev, use_async)


def test_epoch(gpu_lib):
    JC.run_epoch(gpu_lib, dev)


def test_limits(gpu_lib, oracle_lib):
    JC.run_limits(gpu_lib, oracle_lib, dev)


@pytest.mark.parametrize("on_device", (False, True))
def test_python_interface(gpu_lib, oracle_lib, on_device):
    JC.run_python_api(gpu_lib, oracle_lib, dev, on_device)
