"""CPU (hipcc cross-compiles gfx950): the generated code of the second-order transport kernels (csrc/musclkernels.hpp), by the method
of tests/test_advect_isa.py. (1) No instantiation of k_slopes3d / k_advect_muscl3d / k_advflux_muscl3d / k_cf_flux_muscl3d or of the
2D kernels uses scratch memory or spills a register. (2) The marches keep their planes in flight ("hidden
waits"): no wait inside a march sits on the newest request. The floors follow from the request pattern, not from a measurement.
  flux marches   a step requests, in order, its two halo values (c and S), the plane pair of z + 2, the six pairs of S of plane
                 z + 1 and -- behind its fluxes -- the 8 loads of U for the next plane. The next step waits first for the halo values
                 and S (16 and more loads younger), then for U, behind which it has itself requested its halo values, its plane pair
                 and its S set: those ten stay in flight at every wait                                              -> vmcnt >= 10
  slope pass     a step requests its halo value and the plane pair of z + 3; it waits for the halo value of the step before, behind
                 which stands that step's plane pair                                                                -> vmcnt >= 2
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_isa_waits import main_loop, waits_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc", "gmg_muscl.hip")
OURS = ("k_slopes3d", "k_advect_muscl3d", "k_advflux_muscl3d", "k_cf_flux_muscl3d", "k_slopes2d", "k_advect_muscl2d", "k_cf_flux_muscl2d")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("isa") / "muscl.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().split("\n")


def bodies(asm):
    """mangled name -> the lines of the kernel's code, for the kernels of musclkernels.hpp"""
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
    # 3D: the slope pass, the fused march and the flux march at n = 4 (1 slab count), 8 (2), 16 (3), 32 (4), the slot fill at the four
    # sizes; 2D: the slope pass, the march in its two forms, the slot fill
    assert len(ours) == 10 + 10 + 10 + 4 + 1 + 2 + 1, sorted(ours)
    for name, v in ours.items():
        assert v == dict(private_segment_fixed_size=0, sgpr_spill_count=0, vgpr_spill_count=0), (name, v)
    found = bodies(asm)
    assert sorted(found) == sorted(ours)
    for name, body in found.items():
        assert not any("scratch_" in l for l in body), name


# the instantiations at 32^3 and 16^3 whose slab is long enough for the march to be a loop (ZL >= 6; a four-plane slab is
# straight-line code), as in tests/test_advect_isa.py
SIZES = ((32, 1), (32, 2), (32, 4), (16, 1), (16, 2))
MARCHES = [f"{k}ILi{n}ELi{zs}E" for k in ("k_advect_muscl3d", "k_advflux_muscl3d") for n, zs in SIZES]
SLOPES = [f"k_slopes3dILi{n}ELi{zs}E" for n, zs in SIZES]


def march_of(asm, frag):
    found = bodies(asm)
    name = next((n for n in found if frag in n), None)
    assert name is not None, f"{frag} is not instantiated"
    body = found[name]
    s, e = main_loop(body)
    assert sum("s_barrier" in l for l in body[s:e + 1]) == 2, "two plane steps per iteration of the march"
    return body, s, e


@pytest.mark.parametrize("frag", MARCHES)
def test_flux_march_never_waits_for_the_loads_of_its_own_step(asm, frag):
    body, s, e = march_of(asm, frag)
    w = waits_in(body, s, e)
    print(frag, sorted(set(w)))
    assert w and min(w) >= 10, sorted(set(w))
    assert sum("global_load" in l for l in body[s:e + 1]) == 36, "18 loads per step (2 halos, plane pair, 6 of S, 8 of U), none under a branch"


@pytest.mark.parametrize("frag", SLOPES)
def test_slope_pass_never_waits_for_its_newest_request(asm, frag):
    body, s, e = march_of(asm, frag)
    w = waits_in(body, s, e)
    print(frag, sorted(set(w)))
    assert w and min(w) >= 2, sorted(set(w))
    assert sum("global_load" in l for l in body[s:e + 1]) == 6, "3 loads per step (halo, plane pair), none under a branch"
