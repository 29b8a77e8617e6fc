"""Device-side join on the host simulation: the per-slot decisions of the kernels (gobpfld_amd/csrc/xe_mapops.h:
JOIN_SELECT in place of the scan's SELECT, then SCAN, SCATTER, COPY, JOIN_VALUE and EXPIRE) run as loops over host
memory, against a Python join of the oracle's entries of both maps (tests/mapjoin_cases.py). The simulation runs
one slot after another with the plain probe (mo_find), so the diverging grouped probes, the ballots and the
striding waves exist on the device only (tests/test_mapjoin_gpu.py); it still pins down what the right answer is."""
import numpy as np
import pytest

import mapjoin_cases as JC


def dev(a):
    return np.ascontiguousarray(a)


def test_join_restatement():
    JC.check_join_table()


@pytest.mark.parametrize("mode", JC.MODES)
@pytest.mark.parametrize("live", JC.EDGE_COUNTS)
def test_tile_and_round_edges(hostsim_lib, oracle_lib, live, mode):
    JC.run_edges(hostsim_lib, oracle_lib, dev, live, mode)


def test_striding_waves(hostsim_lib, oracle_lib):
    JC.run_striding(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("shape", JC.JOIN_SHAPES)
def test_probe_paths(hostsim_lib, oracle_lib, shape):
    JC.run_shape(hostsim_lib, oracle_lib, dev, shape)


@pytest.mark.parametrize("ks", JC.CHAIN_KEY_SIZES)
def test_chains_in_the_other_map(hostsim_lib, oracle_lib, ks):
    JC.run_chains(hostsim_lib, oracle_lib, dev, ks)


def test_nil_backed_values(hostsim_lib, oracle_lib):
    JC.run_vlen0(hostsim_lib, oracle_lib, dev)


def test_array_sides(hostsim_lib, oracle_lib):
    JC.run_array_sides(hostsim_lib, oracle_lib, dev)


def test_filters(hostsim_lib, oracle_lib):
    JC.run_filters(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("host_form", (False, True))
def test_removal(hostsim_lib, oracle_lib, host_form):
    JC.run_removal(hostsim_lib, oracle_lib, dev, host_form)


def test_removal_writes_the_delta_base(hostsim_lib):
    JC.run_removal_delta(hostsim_lib, dev)


def test_self_join(hostsim_lib, oracle_lib):
    JC.run_self_join(hostsim_lib, oracle_lib, dev)


@pytest.mark.parametrize("use_async", (False, True))
def test_beside_traffic(hostsim_lib, oracle_lib, use_async):
    JC.run_mixed(hostsim_lib, oracle_lib, dev, use_async)


def test_epoch(hostsim_lib):
    JC.run_epoch(hostsim_lib, dev)


def test_limits(hostsim_lib, oracle_lib):
    JC.run_limits(hostsim_lib, oracle_lib, dev)


def test_python_interface(hostsim_lib, oracle_lib):
    JC.run_python_api(hostsim_lib, oracle_lib, dev, False)
