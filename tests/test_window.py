"""The packet header window on the host simulation (the same xe_interp.h the device runs, one lane a wave,
so one wave walks every chunk and both window buffers): the cases of tests/window_cases.py, and the
XE_HDR_LO / XE_HDR_HI the generator gives each read range (xe_jit.cpp packet_read_range, emit_window)."""
import pytest

import window_cases as WC
from test_aot import _window


@pytest.mark.parametrize("tail_gap", (0, 5))
@pytest.mark.parametrize("size", WC.SIZES)
def test_read_sweep(hostsim_lib, oracle_lib, size, tail_gap):
    WC.run_read_sweep(hostsim_lib, oracle_lib, size, tail_gap)


@pytest.mark.parametrize("size", WC.SIZES)
def test_read_sweep_sequential(hostsim_lib, oracle_lib, size):
    WC.run_read_sweep(hostsim_lib, oracle_lib, size, 0, mode=WC.MODE_SEQUENTIAL)


@pytest.mark.parametrize("name", list(WC.shape_programs()))
def test_generated_window(hostsim_lib, name):
    """[lo, hi) of the reads becomes (lo, min(hi, lo + 49)), proven; reads from byte 64 up leave the default
    window; a program reading no packet byte gets the empty window (0, 0)."""
    from gobpfld_amd import aot
    from gobpfld_amd.emulator import ENGINE_JIT, Settings
    srcs = aot.sources([(WC.shape_programs()[name][0], [], None, Settings(engine=ENGINE_JIT))], lib=hostsim_lib)
    assert srcs, "no kernel source generated"
    want = (0, 0) if name == "none" else WC.shape_window(*map(int, name.split("_")))
    assert _window(srcs[0]) == want
    assert ("#define XE_HDR_LO_PROVEN 1" in srcs[0]) == (want is not None)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
@pytest.mark.parametrize("name", list(WC.shape_programs()))
def test_window_shape_programs(hostsim_lib, oracle_lib, name, mode):
    """(On the host every program runs in the interpreter's window [0, 64): this pins the programs and
    their numpy twins against the oracle; the per-program windows are the device's.)"""
    WC.run_window_shape(hostsim_lib, oracle_lib, name, 0, mode=mode)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
def test_umem_tail(hostsim_lib, oracle_lib, mode):
    WC.run_umem_tail(hostsim_lib, oracle_lib, WC.FULL, mode=mode)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
@pytest.mark.parametrize("kind,size", [(k, s) for k, sizes in WC.KINDS.items() for s in sizes])
def test_write_through(hostsim_lib, oracle_lib, kind, size, mode):
    WC.run_write_through(hostsim_lib, oracle_lib, kind, size, mode=mode)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
@pytest.mark.parametrize("name", list(WC.jit_write_programs()))
def test_write_programs_of_the_kernels(hostsim_lib, oracle_lib, name, mode):
    WC.check_ops(hostsim_lib, oracle_lib, name, WC.jit_write_programs()[name], ("flat", 13), *WC.layout_flat(13),
                 WC._settings(0, mode))


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
def test_key_stored_across_the_window_end(hostsim_lib, oracle_lib, mode):
    WC.run_keyed(hostsim_lib, oracle_lib, WC.interp_store_offsets(4), mode=mode)
