"""CPU (hipcc cross-compiles gfx950): the generated code of the transport kernels (csrc/advectkernels.hpp), by the method of
tests/test_density_isa.py. (1) No instantiation of k_advect3d / k_advflux3d / k_cf_flux3d / k_faces_match3d or of the 2D kernels uses
scratch memory or spills a register. (2) The marches keep their planes in flight ("hidden waits"): no
wait inside the march drains the loads the same step has requested. The floor follows from the request pattern, not from a
measurement: a step requests, in order, the halo value, the plane pair of z + 2 and -- behind its fluxes -- the 8 loads of U for
the next plane. The next step waits first for the halo value (10 loads younger), then for U, behind which it has itself requested
its halo value and its plane pair: those three stay in flight at every wait                                         -> vmcnt >= 3
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_isa_waits import main_loop, waits_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc", "gmg_advect.hip")
OURS = ("k_advect3d", "k_advflux3d", "k_cf_flux3d", "k_faces_match3d", "k_advect2d", "k_cf_flux2d", "k_faces_match2d", "k_faces_rate")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("isa") / "advect.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().split("\n")


def bodies(asm):
    """mangled name -> the lines of the kernel's code, for the kernels of advectkernels.hpp"""
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
    # 3D: the fused march and the flux march at n = 4 (1 slab count), 8 (2), 16 (3), 32 (4), the slot fill and the matching at the
    # four sizes; 2D: the march in its two forms, the slot fill, the matching; the rate
    assert len(ours) == 10 + 10 + 4 + 4 + 2 + 1 + 1 + 1, sorted(ours)
    for name, v in ours.items():
        assert v == dict(private_segment_fixed_size=0, sgpr_spill_count=0, vgpr_spill_count=0), (name, v)
    found = bodies(asm)
    assert sorted(found) == sorted(ours)
    for name, body in found.items():
        assert not any("scratch_" in l for l in body), name


# the instantiations at 32^3 and 16^3 whose slab is long enough for the march to be a loop (ZL >= 6; a four-plane slab is
# straight-line code). Not held to this: n = 8, whose three-iteration loop in k_advect3d<8, 1> copies the U set into other registers
# on its back edge and waits for it there (DESIGN.md 23 records it; k_advflux3d<8, 1> does not).
CASES = [f"{k}ILi{n}ELi{zs}E" for k in ("k_advect3d", "k_advflux3d") for n, zs in ((32, 1), (32, 2), (32, 4), (16, 1), (16, 2))]


@pytest.mark.parametrize("frag", CASES)
def test_march_never_waits_for_the_loads_of_its_own_step(asm, frag):
    found = bodies(asm)
    name = next((n for n in found if frag in n), None)
    assert name is not None, f"{frag} is not instantiated"
    body = found[name]
    s, e = main_loop(body)
    assert sum("s_barrier" in l for l in body[s:e + 1]) == 2, "two plane steps per iteration of the march"
    w = waits_in(body, s, e)
    assert w and min(w) >= 3, sorted(set(w))
    assert sum("global_load" in l for l in body[s:e + 1]) == 22, "11 loads per step (halo, plane pair, 8 of U), none under a branch"
