"""The host-simulation loops of the map compaction under ASan/UBSan: a stand-alone program
(tests/sanitize/san_mapcompact.cpp) calls xe_map_compact of the sanitized host-simulation library (the build of
tests/test_sanitize.py, shared with it) on runs placed by hand in tables of 16 to 512 slots, on runs of exactly
kMcMaxRun slots and of one more, and on a table without a free record, and compares the image every call leaves
with a rebuild computed in the program. A sanitizer report fails the test."""
import os
import re
import shutil
import subprocess

import pytest

from test_sanitize import FLAGS, OUT, ROOT, SAN, _build


@pytest.mark.slow
def test_sanitized_map_compact():
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
    src = SAN / "san_mapcompact.cpp"
    prog = _build(OUT / "san_mapcompact", [cxx, *FLAGS, str(src), "-ldl"], [src, ROOT / "include" / "xdpemu.h"])
    max_run = re.search(r"kMcMaxRun = (\d+)", (csrc / "xe_mapops.h").read_text()).group(1)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([str(prog), str(sim), max_run], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "san_mapcompact: 0 failed checks" in r.stdout, r.stdout
