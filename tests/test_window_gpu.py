"""The packet header window on the product library (gfx950: LDS-DMA staging, the double buffer across
chunks, the generated per-program windows): the cases of tests/window_cases.py on the interpreter kernel
and on the per-program kernels."""
import pytest

import window_cases as WC
from gobpfld_amd.emulator import ENGINE_INTERP, ENGINE_JIT

pytestmark = pytest.mark.gpu
ENGINES = [ENGINE_INTERP, ENGINE_JIT]
ENGINE_IDS = ["interp", "jit"]
SHAPE_NAMES = list(WC.shape_programs())


@pytest.mark.parametrize("tail_gap", (0, 5))
@pytest.mark.parametrize("size", WC.SIZES)
def test_read_sweep(gpu_lib, oracle_lib, size, tail_gap):
    WC.run_read_sweep(gpu_lib, oracle_lib, size, tail_gap, engine=ENGINE_INTERP)


@pytest.mark.parametrize("size", WC.SIZES)
def test_read_sweep_sequential(gpu_lib, oracle_lib, size):
    WC.run_read_sweep(gpu_lib, oracle_lib, size, 0, engine=ENGINE_INTERP, mode=WC.MODE_SEQUENTIAL)


@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_window_shapes(gpu_lib, oracle_lib, name, engine):
    for tail_gap in (0, 5):
        WC.run_window_shape(gpu_lib, oracle_lib, name, tail_gap, engine=engine)


@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_window_shapes_sequential(gpu_lib, oracle_lib, name, engine):
    WC.run_window_shape(gpu_lib, oracle_lib, name, 0, engine=engine, mode=WC.MODE_SEQUENTIAL)


@pytest.mark.parametrize("sched", WC.SCHEDULES)
@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("shape", [(0, 14), WC.FULL], ids=["14", "full"])
def test_many_chunks(gpu_lib, shape, engine, sched):
    WC.run_many_chunks(gpu_lib, shape, sched, engine=engine)


@pytest.mark.parametrize("engine,shape", [(ENGINE_INTERP, WC.FULL), (ENGINE_JIT, WC.FULL), (ENGINE_JIT, (47, 64)),
                                          (ENGINE_JIT, (60, 100))], ids=["interp-full", "jit-full", "jit-47_64", "jit-60_100"])
def test_umem_tail(gpu_lib, oracle_lib, engine, shape):
    WC.run_umem_tail(gpu_lib, oracle_lib, shape, engine=engine)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
@pytest.mark.parametrize("kind,size", [(k, s) for k, sizes in WC.KINDS.items() for s in sizes])
def test_write_through(gpu_lib, oracle_lib, kind, size, mode):
    WC.run_write_through(gpu_lib, oracle_lib, kind, size, engine=ENGINE_INTERP, mode=mode)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
@pytest.mark.parametrize("name", list(WC.jit_write_programs()))
def test_write_through_kernels(gpu_lib, oracle_lib, name, mode):
    WC.run_write_through_jit(gpu_lib, oracle_lib, name, mode=mode)


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
def test_key_stored_across_the_window_end(gpu_lib, oracle_lib, engine, mode):
    offs = WC.interp_store_offsets(4) if engine == ENGINE_INTERP else WC.JIT_KEY_OFFS
    WC.run_keyed(gpu_lib, oracle_lib, offs, engine=engine, mode=mode)
