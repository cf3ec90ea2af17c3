"""CPU: one boundary kind per side of the domain (te_hier_build_bc) -- the mask through the C ABI, the numbering of the physical
faces (te_hier_bface_index) on every golden mesh and partition, the yardstick itself (the oracle with mixed masks against the
reference's compiled StarPatchOp / BiCGStab, which take one Neumann flag per side), the host generators, and the host-only units
under the sanitizers with the new entry points driven."""
import glob
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import refslice
from pressurepoissonsolver_amd import capi, problems
from tests import bc_util, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dim", [2, 3])
def test_mask_round_trip(dim):
    m = util.mesh("uniform", 1, dim)
    allbits = (1 << 2 * dim) - 1
    for mask in range(allbits + 1):
        H = capi.Hierarchy(m, 4, neumann_sides=mask)
        assert H.neumann_sides == mask
        assert H.singular == (mask == allbits) and H.neumann == (mask == allbits)
    for bad in (allbits + 1, 1 << 2 * dim, 1 << 7, -1):
        with pytest.raises(capi.TeError) as e:
            capi.Hierarchy(m, 4, neumann_sides=bad)
        assert e.value.code == capi.TE_EINVAL
    # the legacy flag: every side
    assert capi.Hierarchy(m, 4, neumann=True).neumann_sides == allbits and capi.Hierarchy(m, 4).neumann_sides == 0
    assert capi.Hierarchy(m, 4, neumann=True).singular and not capi.Hierarchy(m, 4).singular
    names = ("west", "top") if dim == 3 else ("west", "north")
    assert capi.Hierarchy(m, 4, neumann_sides=names).neumann_sides == (0b100001 if dim == 3 else 0b1001)
    # the placement travels with the mask as with the flag
    assert capi.Hierarchy(m, 4, neumann_sides=1, placement=(16, 32, 0)).placement() == (16.0, 32, 0)


MESHES = [(os.path.basename(p), 2 if os.path.basename(p).startswith("2d") else 3) for p in sorted(glob.glob(os.path.join(util.GOLDEN, "*.bin")))]


@pytest.mark.parametrize("name,dim", MESHES)
@pytest.mark.parametrize("nranks", [1, 2, 4, 8])
def test_bface_index_is_the_patch_side_enumeration(name, dim, nranks):
    m = util.mesh(name, 0, dim)
    hs = [capi.Hierarchy(m, 4, neumann_sides=0b0101, rank=r, nranks=nranks) for r in range(nranks)]
    for l in range(hs[0].num_levels):
        t = hs[0].tables(l)
        seen = []
        for H in hs:
            l2g, idx = H.l2g(l), H.bface_index(l)
            want = np.full((len(l2g), 2 * dim), -1, np.int32)
            k = 0
            for p, gp in enumerate(l2g):
                for s in range(2 * dim):
                    if t["nbr_kind"][gp, s] == 0:
                        want[p, s] = k
                        k += 1
                        seen.append((int(gp), s))
            assert np.array_equal(idx, want) and H.num_bfaces(l) == k, (l, H.rank)
        faces = [(int(p), s) for p in range(len(t["id"])) for s in range(2 * dim) if t["nbr_kind"][p, s] == 0]
        if hs[0].replicated(l):  # every rank numbers the whole level
            assert sorted(seen) == sorted(faces * nranks)
        else:  # the ranks' faces partition the level's
            assert sorted(seen) == faces


CASES = [("2refine.bin", 8, 0, 3), ("multi_refine.bin", 4, 0, 3), ("2d2ref.bin", 16, 1, 2)]


@pytest.mark.skipif(not refslice.available(), reason="oracle/_ref/libte_ref.so (the reference's compiled slice) not built")
@pytest.mark.parametrize("name,n,div,dim", CASES)
def test_oracle_with_mixed_masks_equals_the_reference(name, n, div, dim):
    """what licenses the GPU tests: StarPatchOp with one Neumann flag per side (oracle/ref_driver.cpp pi->neumann[s]) against the
    oracle with the same per-patch mask"""
    for mask in (bc_util.MASKS3 if dim == 3 else bc_util.MASKS2):
        m, H, levels = bc_util.setup(name, n, div, mask, dim)
        L = levels[0]
        u = util.rand_vec(L.size, 77)
        assert np.abs(orc.apply(L, u) - refslice.apply(L, u)).max() <= util.op_tol(L, u), bin(mask)
        assert np.abs(orc.patch_apply(L, u) - refslice.patch_apply(L, u)).max() <= util.op_tol(L, u), bin(mask)


@pytest.mark.skipif(not refslice.available(), reason="oracle/_ref/libte_ref.so (the reference's compiled slice) not built")
@pytest.mark.parametrize("name,n,div,dim", [("2refine.bin", 4, 0, 3), ("multi_refine.bin", 4, 0, 3), ("2d2ref.bin", 8, 0, 2)])
def test_oracle_bicgstab_with_mixed_masks_equals_the_reference(name, n, div, dim):
    """the reference's BiCGStab<D>::solve on its own operator against the oracle's, unpreconditioned (the bounds of
    tests/test_oracle_golden.py::test_bicgstab_against_reference)"""
    for mask in (bc_util.MASKS3 if dim == 3 else bc_util.MASKS2):
        m, H, levels = bc_util.setup(name, n, div, mask, dim)
        L = levels[0]
        b = util.rand_vec(L.size, 78)
        x_ref, its_ref = refslice.bicgstab(L, b)
        x, its, rr = orc.bicgstab([L], orc.cycle_opts(), b, use_prec=False)
        assert rr <= 1e-12
        assert abs(its - its_ref) <= max(3, its_ref // 10), (bin(mask), its, its_ref)
        assert np.linalg.norm(x - x_ref) <= 1e-9 * np.linalg.norm(x_ref), bin(mask)


@pytest.mark.parametrize("name,n,div", [("2refine.bin", 8, 0), ("uniform", 4, 2)])
def test_init_sides_equals_the_legacy_generators_bit_for_bit(name, n, div):
    t = capi.Hierarchy(util.mesh(name, div), n).tables(0)
    for problem in ("trig", "gauss"):
        for mask, legacy in ((0, problems.init_dirichlet), (0b111111, problems.init_neumann)):
            f, e = problems.init_sides(t, n, mask, problem)
            wf, we = legacy(t, n, problem)
            assert np.array_equal(f, wf) and np.array_equal(e, we)
    t2 = capi.Hierarchy(util.mesh("2d2ref.bin", 1, 2), n).tables(0)
    f, e = problems.init_sides_2d(t2, n, 0)
    wf, we = problems.init_dirichlet_2d(t2, n)
    assert np.array_equal(f, wf) and np.array_equal(e, we)


def fold_numpy(tables, n, mask, bdata, f, dim, patches=None, largest=None):
    """the fold of a boundary vector into f in plain numpy: one term per physical side, in side order. largest (optional, an
    array like f holding |f| on entry): receives the largest absolute term of every cell"""
    if patches is None:
        patches = np.arange(len(tables["id"]))
    f = f.reshape((len(patches),) + (n,) * dim).copy()
    if largest is not None:
        largest = largest.reshape(f.shape)
    nf, k = n ** (dim - 1), 0
    for i, p in enumerate(patches):
        h = tables["lengths"][p] / n
        for s in range(2 * dim):
            if tables["nbr_kind"][p, s] != 0:
                continue
            ax, up = s // 2, s & 1
            sl = [slice(None)] * dim
            sl[dim - 1 - ax] = -1 if up else 0
            b = bdata[k * nf:(k + 1) * nf].reshape((n,) * (dim - 1))
            k += 1
            term = (-1.0 if up else 1.0) * (b / h[ax]) if (mask >> s) & 1 else -(2 * b / h[ax] ** 2)
            f[i][tuple(sl)] += term
            if largest is not None:
                largest[i][tuple(sl)] = np.maximum(largest[i][tuple(sl)], np.abs(term))
    return f.ravel()


@pytest.mark.parametrize("name,n,div,dim", [("2refine.bin", 8, 0, 3), ("uniform", 4, 1, 3), ("2d2ref.bin", 8, 1, 2)])
def test_boundary_data_folded_on_the_host_is_init_sides(name, n, div, dim):
    """problems.boundary_data is in boundary-vector layout: folding it into the interior right-hand side gives init_sides"""
    for mask in (bc_util.MASKS3 if dim == 3 else bc_util.MASKS2):
        t = capi.Hierarchy(util.mesh(name, div, dim), n, neumann_sides=mask).tables(0)
        init = problems.init_sides if dim == 3 else problems.init_sides_2d
        want, _ = init(t, n, mask)
        interior = dict(t, nbr_kind=np.ones_like(t["nbr_kind"]))  # (no physical face: the right-hand side at the cell centres alone)
        f0, _ = init(interior, n, mask)
        got = fold_numpy(t, n, mask, problems.boundary_data(t, n, mask, dim=dim), f0, dim)
        assert np.abs(got - want).max() <= 4 * util.EPS * np.abs(want).max()


def test_host_units_with_the_boundary_entry_points_are_clean_under_sanitizers():
    """csrc/mesh.cpp and capi_mesh.cpp with -fsanitize=address,undefined, te_hier_build_bc / te_hier_neumann_sides /
    te_hier_singular / te_hier_num_bfaces / te_hier_bface_index driven over refined meshes and 1 / 2 / 3 / 8 ranks
    (tests/bc_sanitize.cpp)"""
    csrc = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bc_sanitize")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "bc_sanitize.cpp"),
                            os.path.join(csrc, "capi_mesh.cpp"), os.path.join(csrc, "mesh.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        args = []
        for name, dim, div in (("2refine.bin", 3, 1), ("multi_refine.bin", 3, 0), ("2d2ref.bin", 2, 2), ("1uni.bin", 3, 2)):
            args += [os.path.join(util.GOLDEN, name), str(dim), str(div)]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0 and "SANITIZE_OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
