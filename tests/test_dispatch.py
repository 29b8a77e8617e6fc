"""Verdict dispatch and TX gather (include/xdpemu_io.h, output side) on the host simulation: the C ABI
and gobpfld_amd.dispatch against the numpy reference of dispatch_cases.py, for exact equality."""
import inspect
import re
from pathlib import Path

import pytest

import dispatch_cases as DC
from gobpfld_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent


def test_constants_match_the_header():
    text = (ROOT / "include" / "xdpemu_io.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define (XE_ACT_[A-Z]+|XE_DISPATCH_TILE) (\d+)", text)}
    assert defs["XE_DISPATCH_TILE"] == N.XE_DISPATCH_TILE
    assert [defs[f"XE_ACT_{k}"] for k in ("ABORTED", "DROP", "PASS", "TX", "REDIRECT", "COUNT")] == [
        N.ACT_ABORTED, N.ACT_DROP, N.ACT_PASS, N.ACT_TX, N.ACT_REDIRECT, N.ACT_COUNT]
    import ctypes as C
    assert C.sizeof(N.DispatchCounts) == 32


@pytest.mark.parametrize("n", DC.SIZES)
def test_dispatch_equals_numpy(hostsim_lib, n):
    DC.check_dispatch(hostsim_lib, False, n)


@pytest.mark.parametrize("ver_offset", (1, 2, 3))
@pytest.mark.parametrize("n", DC.UNALIGNED_SIZES)
def test_dispatch_unaligned_verdicts(hostsim_lib, n, ver_offset):
    DC.check_dispatch(hostsim_lib, False, n, names=("uniform", "failed10"), ver_offset=ver_offset)


def test_dispatch_argument_errors(hostsim_lib):
    DC.check_errors(hostsim_lib, False)


@pytest.mark.parametrize("room", DC.STRIDE_ROOMS)
def test_gather_grid_stride(hostsim_lib, room):
    DC.check_gather_stride(hostsim_lib, False, room)


@pytest.mark.parametrize("room", DC.ROOMS)
def test_gather_matrix_and_bounds(hostsim_lib, room):
    DC.check_gather(hostsim_lib, False, room)


def test_run_pcap_dispatch_is_off_by_default():
    from gobpfld_amd import xsk as X
    assert inspect.signature(X.run_pcap).parameters["dispatch"].default is False
    assert X.PcapRun().action_count is None
