"""CPU (hipcc cross-compiles gfx950): the generated code of the face-vector transfer (csrc/faceregridkernels.hpp) -- every
instantiation of k_facexfer3d / k_facexfer2d uses no scratch memory, spills no register and keeps its static LDS within 64 KiB; the
32^3 refine branch stages one component's block of (H + 1)(H + 2)^2 doubles, H = 16. Reads the kernels' metadata records only."""
from tests.test_fmg_isa import clean, metadata


def test_face_transfer_no_scratch_no_spills_and_lds_fits(tmp_path):
    ours = {k: v for k, v in metadata(tmp_path, "gmg_faceregrid.hip").items() if "k_facexfer" in k}
    three, two = {k: v for k, v in ours.items() if "k_facexfer3d" in k}, {k: v for k, v in ours.items() if "k_facexfer2d" in k}
    assert len(three) == 10, sorted(three)  # n = 4 (1 slab count), 8 (2), 16 (3), 32 (4)
    assert len(two) == 1, sorted(two)
    for name, v in ours.items():
        print(name, v)
        clean(name, v)
    lds32 = next(v["lds"] for k, v in three.items() if "k_facexfer3dILi32ELi1E" in k)
    assert lds32 == 17 * 18 * 18 * 8  # one component over an octant of a 32^3 patch, tangential rings included
    assert all(v["lds"] == 0 for v in two.values())
