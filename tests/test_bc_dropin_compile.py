"""CPU, where the reference tree is present: a translation unit that uses LevelGeometry::neumann_sides and initSides /
initSides2d (pressurepoissonsolver_amd/thunderegg/HipInit.h) compiles against the reference's own headers
(tests/bc_compile.cpp; nothing is run)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("THUNDEREGG_REF", "/root/reference")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src", "Thunderegg")), reason="reference tree not present")
def test_init_sides_compiles_against_reference_headers():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-w", "-I" + os.path.join(REF, "src"), "-I/opt/conda/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pressurepoissonsolver_amd", "thunderegg"),
           os.path.join(ROOT, "tests", "bc_compile.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
