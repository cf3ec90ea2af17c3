"""CPU: the level tables are decided by a host-only unit (pressurepoissonsolver_amd/csrc/level_tables.cpp), so what the kernels and
the exchanges take for granted about them is checked here without a device, for every rank of 1, 2, 4 and 8-rank partitions at once
(tests/level_tables_check.cpp says what is checked). The system g++ is driven directly, with nothing of ROCm on the include path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")
UNITS = ("level_tables.cpp", "mesh.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on this machine")


def _compile(tmp_path):
    objs = []
    for unit in UNITS:
        obj = str(tmp_path / (os.path.splitext(unit)[0] + ".o"))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-c", os.path.join(CSRC, unit), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    return objs


def test_table_builder_compiles_without_rocm(tmp_path):
    """the property everything else rests on: the plain host compiler, no ROCm include path, no device header in the unit"""
    _compile(tmp_path)
    for name in ("level_tables.cpp", "level_tables.hpp", "table_layout.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            includes = [ln for ln in f if ln.lstrip().startswith("#include")]
        assert not any("hip" in ln.lower() or "rccl" in ln.lower() for ln in includes), (name, includes)


def test_level_tables_hold_their_invariants_on_1_2_4_8_ranks(tmp_path):
    exe = str(tmp_path / "level_tables_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", os.path.join(ROOT, "tests", "level_tables_check.cpp")] + _compile(tmp_path) + ["-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("OK "), r.stdout
