"""The host-simulation loops of the map group-by under ASan/UBSan: a stand-alone program
(tests/sanitize/san_mapgroup.cpp) calls xe_map_group of the sanitized host-simulation library (the build of
tests/test_sanitize.py, shared with it) with group bytes and measures at odd offsets, every destination record
size, destinations with exactly enough room and with one entry too little, and compares what the destinations
hold with an aggregate of the source's scanned entries computed in the program. A sanitizer report fails the
test."""
import os
import shutil
import subprocess

import pytest

from test_sanitize import FLAGS, OUT, ROOT, SAN, _build


@pytest.mark.slow
def test_sanitized_map_group():
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
    src = SAN / "san_mapgroup.cpp"
    prog = _build(OUT / "san_mapgroup", [cxx, *FLAGS, str(src), "-ldl"], [src, ROOT / "include" / "xdpemu.h"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([str(prog), str(sim)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "san_mapgroup: 0 failed checks" in r.stdout, r.stdout
