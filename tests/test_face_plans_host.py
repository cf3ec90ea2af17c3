"""CPU: the face-sized transfer plans of the host-only table builder (pressurepoissonsolver_amd/csrc/level_tables.cpp: up_foff,
down_foff, tx_fup), which the restriction of the coefficient uses when children and parents live on different ranks. Checked without
a device for every rank of 1, 2, 3, 4 and 8-rank partitions and the three placements of the small levels at once
(tests/face_plans_check.cpp says what is checked). The system g++ is driven directly, with nothing of ROCm on the include path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")
UNITS = ("level_tables.cpp", "mesh.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on this machine")


def test_face_plans_are_symmetric_and_in_bounds_on_1_2_3_4_8_ranks(tmp_path):
    exe = str(tmp_path / "face_plans_check")
    srcs = [os.path.join(ROOT, "tests", "face_plans_check.cpp")] + [os.path.join(CSRC, u) for u in UNITS]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1"] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("OK "), r.stdout
