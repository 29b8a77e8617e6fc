"""The host-simulation loops of the in-place map edits under ASan/UBSan: a stand-alone program
(tests/sanitize/san_mapmodify.cpp) calls xe_map_modify* of the sanitized host-simulation library (the build of
tests/test_sanitize.py, shared with it) with output buffers of exactly the bytes a call may write, fields at odd
offsets and at the last bytes of odd-sized values, and compares what every call leaves with xe_map_dump edited
in the program. A sanitizer report fails the test."""
import os
import shutil
import subprocess

import pytest

from test_sanitize import FLAGS, OUT, ROOT, SAN, _build


@pytest.mark.slow
def test_sanitized_map_modify():
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
    src = SAN / "san_mapmodify.cpp"
    prog = _build(OUT / "san_mapmodify", [cxx, *FLAGS, str(src), "-ldl"], [src, ROOT / "include" / "xdpemu.h"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([str(prog), str(sim)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "san_mapmodify: 0 failed checks" in r.stdout, r.stdout
