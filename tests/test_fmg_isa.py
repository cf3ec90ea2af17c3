"""CPU (hipcc cross-compiles gfx950): the generated code of te_fmg's own kernels -- the quadratic FMG interpolation
(csrc/prolongkernels.hpp k_prolong_quadratic3d / 2d) and the restriction of boundary vectors (csrc/bckernels.hpp
k_boundary_restrict). No instantiation uses scratch memory or spills a register, and the staged ring block fits the 64 KiB of
static LDS. Reads the kernels' metadata records only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")


def metadata(tmp, unit):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = tmp / (unit + ".s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", os.path.join(CSRC, unit), "-o", str(out)],
                   check=True, capture_output=True, timeout=900)
    meta, cur, lds = {}, {}, 0
    for l in out.read_text().split("\n"):  # fields in alphabetical order: the LDS size, then .name, then the other sizes
        m = re.match(r"^\s+\.(name|group_segment_fixed_size|private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count|vgpr_count):\s+(\S+)", l)
        if not m:
            continue
        if m.group(1) == "group_segment_fixed_size":
            lds = int(m.group(2))
        elif m.group(1) == "name":
            cur = meta.setdefault(m.group(2), dict(lds=lds))
        else:
            cur[m.group(1)] = int(m.group(2))
    return meta


def clean(name, v):
    assert (v["private_segment_fixed_size"], v["sgpr_spill_count"], v["vgpr_spill_count"]) == (0, 0, 0), (name, v)
    assert v["lds"] <= 64 * 1024, (name, v)


def test_quadratic_prolongation_no_scratch_no_spills_and_lds_fits(tmp_path):
    ours = {k: v for k, v in metadata(tmp_path, "gmg_prolong.hip").items() if "k_prolong_quadratic" in k}
    assert len(ours) == 11, sorted(ours)  # 3D: n = 4 (1 slab count), 8 (2), 16 (3), 32 (4); 2D: one kernel
    for name, v in ours.items():
        print(name, v)
        clean(name, v)
    lds32 = next(v["lds"] for k, v in ours.items() if "k_prolong_quadratic3dILi32ELi1E" in k)
    assert lds32 == 18 ** 3 * 8  # the ring block of an octant of a 32^3 patch: no wider than the linear interpolator's


def test_boundary_restriction_no_scratch_no_spills(tmp_path):
    ours = {k: v for k, v in metadata(tmp_path, "gmg_bc.hip").items() if "k_boundary_restrict" in k}
    assert len(ours) == 2, sorted(ours)
    for name, v in ours.items():
        print(name, v)
        clean(name, v)
        assert v["lds"] == 0
