"""CPU (hipcc cross-compiles gfx950): the generated code of the variable-density kernels (csrc/densitykernels.hpp), by the metadata
method of tests/test_projection_isa.py. (1) No instantiation of k_cellface3d / k_wproject3d / k_cf_raw3d / k_cellface2d /
k_wproject2d / k_cf_raw2d / k_boundary_rhs_w uses scratch memory or spills a register -- k_wproject3d streams two face vectors
beside the cell planes and still has to fit. (2) The plane marches keep their planes in flight ("hidden
waits"): no wait inside the march drains the loads the same step has requested. The floors follow from the request pattern, not
from a measurement:
  cellface   k_gradient3d<N, false>'s pattern: the halo value is requested one step ahead, first in its step; behind it the step
             requests the plane pair of z + 2, which nothing touches for two steps                                    -> vmcnt >= 2
  wproject   a step's requests, in order: the halo value and its boundary term, the plane pair of z + 2, and -- behind its stores --
             the 16 loads of U and w for the next plane. The next step waits first for the halo pair (18 loads and 8 stores
             younger), then for U and w, behind which it has itself requested only its halo pair and its plane pair: those four
             stay in flight at every wait                                                                              -> vmcnt >= 4
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_isa_waits import main_loop, waits_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc", "gmg_density.hip")
OURS = ("k_cellface3d", "k_wproject3d", "k_cf_raw3d", "k_cellface2d", "k_wproject2d", "k_cf_raw2d", "k_boundary_rhs_w")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("isa") / "density.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().split("\n")


def bodies(asm):
    """mangled name -> the lines of the kernel's code, for the kernels of densitykernels.hpp"""
    starts = [(i, l.split(":")[0]) for i, l in enumerate(asm) if re.match(r"^_ZN2te\w+:", l)]
    out = {}
    for k, (i, name) in enumerate(starts):
        if any(o in name for o in OURS):
            j = starts[k + 1][0] if k + 1 < len(starts) else len(asm)
            out[name] = asm[i:next((e for e in range(i, j) if asm[e].startswith(".Lfunc_end")), j)]
    return out


def test_no_scratch_and_no_spills(asm):
    meta, cur = {}, {}
    for l in asm:  # the kernels' metadata records: fields in alphabetical order, .name before the sizes it belongs to
        m = re.match(r"^\s+\.(name|private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", l)
        if not m:
            continue
        if m.group(1) == "name":
            cur = meta.setdefault(m.group(2), {})
        else:
            cur[m.group(1)] = int(m.group(2))
    ours = {k: v for k, v in meta.items() if any(o in k for o in OURS)}
    # 3D: cellface and wproject at n = 4 (1 slab count), 8 (2), 16 (3), 32 (4), the raw coarse/fine fill at the four sizes;
    # 2D: three kernels; the weighted fold in 2D and 3D
    assert len(ours) == 10 + 10 + 4 + 3 + 2, sorted(ours)
    for name, v in ours.items():
        assert v == dict(private_segment_fixed_size=0, sgpr_spill_count=0, vgpr_spill_count=0), (name, v)
    found = bodies(asm)
    assert sorted(found) == sorted(ours)
    for name, body in found.items():
        assert not any("scratch_" in l for l in body), name


# every instantiation whose slab is long enough for the march to be a loop (ZL >= 6; a four-plane slab is straight-line code)
CASES = [("k_cellface3dILi32ELi1E", 2), ("k_cellface3dILi32ELi2E", 2), ("k_cellface3dILi32ELi4E", 2), ("k_cellface3dILi16ELi1E", 2),
         ("k_cellface3dILi16ELi2E", 2), ("k_cellface3dILi8ELi1E", 2),
         ("k_wproject3dILi32ELi1E", 4), ("k_wproject3dILi32ELi2E", 4), ("k_wproject3dILi32ELi4E", 4), ("k_wproject3dILi16ELi1E", 4),
         ("k_wproject3dILi16ELi2E", 4), ("k_wproject3dILi8ELi1E", 4)]


@pytest.mark.parametrize("frag,floor", CASES, ids=[c[0] for c in CASES])
def test_march_never_waits_for_the_loads_of_its_own_step(asm, frag, floor):
    found = bodies(asm)
    name = next((n for n in found if frag in n), None)
    assert name is not None, f"{frag} is not instantiated"
    body = found[name]
    s, e = main_loop(body)
    assert sum("s_barrier" in l for l in body[s:e + 1]) == 2, "two plane steps per iteration of the march"
    w = waits_in(body, s, e)
    assert w and min(w) >= floor, sorted(set(w))
    assert sum("global_load" in l for l in body[s:e + 1]) == (6 if "cellface" in frag else 40), "3 / 20 loads per step, none under a branch"
