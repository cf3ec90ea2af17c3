"""CPU (hipcc cross-compiles gfx950): the generated code of the MAC kernels (csrc/projkernels.hpp). (1) No instantiation of
k_gradient3d / k_divergence3d / k_gradient2d / k_divergence2d uses scratch memory or spills a register. (2) The plane marches keep
their planes in flight ("hidden waits", as tests/test_isa_waits.py checks it for the cycle's kernels): no wait inside
the march drains the loads the same step has requested. The floors follow from the request pattern, not from a measurement:
  divergence   a step requests 8 loads (2 x LO_x, LO_y, LO_z, HI_x, HI_y) and consumes only what was requested two steps earlier:
               the 8 loads of the step before may all still be in flight at every wait                                -> vmcnt >= 8
  gradient     the halo value (and its boundary term) is requested one step ahead, first in its step, as in k_stencil3d; behind it
               the step requests the plane pair of z + 2, which nothing touches for two steps                          -> vmcnt >= 2
  project      the same, with the 8 loads of U behind the halo                                                        -> vmcnt >= 2
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_isa_waits import main_loop, waits_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc", "gmg_projection.hip")
OURS = ("k_gradient3d", "k_divergence3d", "k_gradient2d", "k_divergence2d")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("isa") / "proj.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().split("\n")


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
    # 3D: gradient and project at n = 4 (1 slab count), 8 (2), 16 (3), 32 (4) and the divergence at the same ten; 2D: three kernels
    assert len(ours) == 33, sorted(ours)
    for name, v in ours.items():
        assert v == dict(private_segment_fixed_size=0, sgpr_spill_count=0, vgpr_spill_count=0), (name, v)
    text = "\n".join(asm)
    for o in OURS:
        for body in re.findall(r"^_ZN2te\d+" + o + r"\w*:\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M):
            assert "scratch_" not in body, o


CASES = [("k_gradient3dILi32ELb0ELi1E", 2), ("k_gradient3dILi32ELb1ELi1E", 2), ("k_gradient3dILi16ELb0ELi2E", 2),
         ("k_divergence3dILi32ELi1E", 8), ("k_divergence3dILi16ELi2E", 8), ("k_divergence3dILi8ELi1E", 8)]


@pytest.mark.parametrize("frag,floor", CASES, ids=[c[0] for c in CASES])
def test_march_never_waits_for_the_loads_of_its_own_step(asm, frag, floor):
    starts = [(i, l.split(":")[0]) for i, l in enumerate(asm) if re.match(r"^_ZN2te\w+:", l)]
    k = next((k for k, (i, n) in enumerate(starts) if frag in n), None)
    assert k is not None, f"{frag} is not instantiated"
    i = starts[k][0]
    j = starts[k + 1][0] if k + 1 < len(starts) else len(asm)
    body = asm[i:next((e for e in range(i, j) if asm[e].startswith(".Lfunc_end")), j)]
    s, e = main_loop(body)
    assert sum("s_barrier" in l for l in body[s:e + 1]) == 2, "two plane steps per iteration of the march"
    w = waits_in(body, s, e)
    assert w and min(w) >= floor, sorted(set(w))
