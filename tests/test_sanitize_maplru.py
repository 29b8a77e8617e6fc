"""The host-simulation loops of the device-side LRU_HASH calls under ASan/UBSan: a stand-alone program
(tests/sanitize/san_maplru.cpp) calls xe_lru_lookup_batch_device, xe_lru_delete_batch_device, xe_lru_order_device,
xe_lru_evict_device and the host-pointer forms of the sanitized host-simulation library (the build of
tests/test_sanitize.py, shared with it) with keys of 4, 13 and 64 bytes, values of every sub-group width, batches
and outputs in heap blocks of exactly their size, k below, at and above matched, filters on odd fields, deletes
with repetitions and evictions, and compares every answer with a model of the usage list kept in the program. A
sanitizer report fails the test."""
import os
import shutil
import subprocess

import pytest

from test_sanitize import FLAGS, OUT, ROOT, SAN, _build


@pytest.mark.slow
def test_sanitized_map_lru():
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ missing")
    OUT.mkdir(exist_ok=True)
    csrc = ROOT / "gobpfld_amd" / "csrc"
    hdrs = sorted(csrc.glob("*.h")) + [ROOT / "include" / "xdpemu.h", ROOT / "include" / "xdpemu_io.h"]
    from gobpfld_amd.build import HOSTSIM_UNITS
    sim_src = [csrc / u for u in HOSTSIM_UNITS]
    sim = _build(OUT / "libxdpemu_hostsim_san.so",
                 [cxx, *FLAGS, "-fPIC", "-shared", "-DXE_HOSTSIM", "-DXE_HOSTSIM_POISON", *map(str, sim_src), "-pthread"], sim_src + hdrs)
    src = SAN / "san_maplru.cpp"
    prog = _build(OUT / "san_maplru", [cxx, *FLAGS, str(src), "-ldl"], [src, ROOT / "include" / "xdpemu.h"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([str(prog), str(sim)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "san_maplru: 0 failed checks" in r.stdout, r.stdout
