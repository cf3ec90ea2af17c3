"""CPU (hipcc cross-compiles gfx950): the generated code of the regridding kernels (csrc/regridkernels.hpp) -- every instantiation of
k_regrid3d / k_regrid2d and of the indicator kernels uses no scratch memory and spills no register, and the static LDS of the
32^3 refine branch is one ring block of 18^3 doubles. Reads the kernels' metadata records only."""
from tests.test_fmg_isa import clean, metadata


def test_regrid_and_indicator_no_scratch_no_spills(tmp_path):
    meta = metadata(tmp_path, "gmg_regrid.hip")
    regrid = {k: v for k, v in meta.items() if "k_regrid" in k}
    indicator = {k: v for k, v in meta.items() if "k_indicator" in k}
    assert len(regrid) == 11, sorted(regrid)  # 3D: n = 4 (1 slab count), 8 (2), 16 (3), 32 (4); 2D: one kernel
    assert len(indicator) == 12, sorted(indicator)  # the same ten, the 2D kernel and the fixed-order final maximum
    for name, v in {**regrid, **indicator}.items():
        print(name, v)
        clean(name, v)
    lds32 = next(v["lds"] for k, v in regrid.items() if "k_regrid3dILi32ELi1E" in k)
    assert lds32 == 18 ** 3 * 8  # the ring block of an octant of a 32^3 patch
    assert all(v["lds"] <= 32 for v in indicator.values())  # one partial maximum per wave
