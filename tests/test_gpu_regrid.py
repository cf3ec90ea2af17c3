"""-m gpu: adaptive regridding on the device -- te_patch_indicator and te_vec_regrid against their numpy statements
(tests/regrid_util.py; the statements themselves are checked on the CPU by tests/test_regrid_host.py), and the adapted meshes as
inputs to the whole stack (operator, cycle, Krylov solve against the oracle).

Tolerances. Indicator: bit for bit ((a + b) - 2 c does not depend on FMA contraction, a maximum not on order). Transfer: copied patches
bit for bit; coarsened patches bit for bit against te_restrict on the SOURCE solver; refined patches |delta| <= 32 eps 1.75^D max|e|, e
the source patch -- a ghost of the extended block carries weight 3 + 3 + 1 = 7 and enters through the -3/32 tap, so the sum of absolute
weights per axis is at most (30 + 5 + 21) / 32 = 1.75, and a wrong weight or source cell is off by O(0.1 max|e|). Operator: util.op_tol;
cycle: 1e-10 relative, the project's cycle tolerance."""
import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi
from tests import regrid_util as ru, util

pytestmark = pytest.mark.gpu

# (mesh, n, divides, dim): the smallest patch, a z-slab size with several blocks, the production patch size (8 -> 64 patches of 32^3:
# eight slabs per patch by stencilSlabs), coarse/fine trees at a four-slab size and five levels deep, the 2D kernel on a tree and at
# 64^2. One slab per patch: the rule gives it from 2048 patches on (test_one_slab_per_patch below); on few patches TE_ZS_PIN gives it and
# every other admitted count (tests/test_gpu_slab_matrix.py).
SHAPES = [("uniform", 4, 2, 3), ("uniform", 8, 2, 3), ("uniform", 32, 1, 3), ("2refine.bin", 16, 0, 3), ("multi_refine.bin", 8, 0, 3),
          ("2d2ref.bin", 4, 0, 2), ("uniform", 64, 2, 2)]


def mixed(m):
    """+1 on one corner family, -1 on the opposite one; on a one-family mesh (uniform d = 1): +1 on one leaf"""
    if len(m.leaves()) == 1 << m.dim:
        return {int(m.leaves()[0]): 1}
    return ru.mixed_flags(m)


def flags(m, pattern):
    return mixed(m) if pattern == "mixed" else {int(i): int(pattern) for i in m.leaves()}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda c: f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}d")
def case(request):
    name, n, div, dim = request.param
    orc.set_threads(16)
    m = util.mesh(name, div, dim)
    H = capi.Hierarchy(m, n)
    return dict(name=name, n=n, dim=dim, m=m, H=H, g=capi.GMG(H), adapted={})


def adapted(case, pattern):
    if pattern not in case["adapted"]:
        m2 = case["m"].adapt(flags(case["m"], pattern))
        H2 = capi.Hierarchy(m2, case["n"])
        case["adapted"][pattern] = dict(m=m2, H=H2, g=capi.GMG(H2))
    return case["adapted"][pattern]


def test_indicator_every_level_bit_for_bit(case):
    g, H, n, dim = case["g"], case["H"], case["n"], case["dim"]
    for l in range(H.num_levels):
        P = H.sizes(l)[0]
        u = util.rand_vec(P * n ** dim, 30 + l)
        du = g.new_vector(l, u)
        got = g.patch_indicator(du, level=l)
        assert np.array_equal(got, ru.indicator(u, P, n, dim)), l
        assert np.array_equal(du.download(), u), l


def test_indicator_on_two_virtual_ranks(case):
    """patch-local, so a sharded hierarchy gives its local patches' values: concatenated through l2g they are the single-rank output"""
    g, H, n, dim = case["g"], case["H"], case["n"], case["dim"]
    hs = [capi.Hierarchy(case["m"], n, rank=r, nranks=2) for r in range(2)]
    gs = [capi.GMG(h) for h in hs]
    for l in range(min(H.num_levels, hs[0].num_levels)):
        P = H.sizes(l)[1]
        u = util.rand_vec(P * n ** dim, 40 + l).reshape(P, -1)
        one = g.patch_indicator(g.new_vector(l, u), level=l)
        both, seen = np.full(P, -1.0), 0
        for h, gr in zip(hs, gs):
            l2g = h.l2g(l)
            if len(l2g) == 0:
                continue
            both[l2g] = gr.patch_indicator(gr.new_vector(l, u[l2g]), level=l)
            seen += len(l2g)
        assert seen >= P and np.array_equal(both, one), l


@pytest.mark.parametrize("pattern", ["+1", "-1", "mixed"])
def test_transfer(case, pattern):
    g, H, n, dim = case["g"], case["H"], case["n"], case["dim"]
    A = adapted(case, pattern)
    u = util.rand_vec(H.cells(0), 50)
    us, ud = g.new_vector(0, u), A["g"].new_vector(0)
    ud.set(123.0)
    capi.regrid(g, us, A["g"], ud)
    got = ud.download().reshape(A["H"].sizes(0)[0], -1)
    want, kinds = ru.regrid(H.leaf_tree(), A["H"].leaf_tree(), u, n, dim)
    want = want.reshape(got.shape)
    assert np.array_equal(us.download(), u)
    print(f"{pattern}: copy {(kinds == ru.COPY).sum()} refine {(kinds == ru.REFINE).sum()} coarsen {(kinds == ru.COARSEN).sum()}")
    if pattern == "mixed" and case["name"] == "uniform" and len(case["m"].leaves()) > 1 << dim:
        assert all((kinds == k).any() for k in (ru.COPY, ru.REFINE, ru.COARSEN))
    if pattern == "+1":
        assert (kinds == ru.REFINE).all()
    if pattern == "-1" and case["name"] == "uniform":
        assert (kinds == ru.COARSEN).all()
    # te_restrict on the source solver, level by level: a coarsened parent is a patch of the first coarser level that lists its id
    restricted = [us]
    for l in range(H.num_levels - 1):
        restricted.append(g.new_vector(l + 1))
        g.restrict(restricted[l + 1], restricted[l], fine_level=l)
    level_ids = [H.tables(l)["id"] for l in range(H.num_levels)]
    src_leaf = {int(i): p for p, i in enumerate(H.leaf_tree()["id"])}
    dst = A["H"].leaf_tree()
    uv, worst = u.reshape(H.sizes(0)[0], -1), 0.0
    for p, k in enumerate(kinds):
        i = int(dst["id"][p])
        if k == ru.COPY:
            assert np.array_equal(got[p], uv[src_leaf[i]]), ("copy", i)
        elif k == ru.COARSEN:
            l = next(l for l in range(1, H.num_levels) if i in level_ids[l])
            q = int(np.flatnonzero(level_ids[l] == i)[0])
            assert np.array_equal(got[p], restricted[l].download_patches(q, 1)), ("coarsen", i)
            assert np.array_equal(got[p], want[p]), ("coarsen statement", i)
        else:
            e = uv[src_leaf[int(dst["tree_parent"][p])]]
            err, bound = np.abs(got[p] - want[p]).max(), 32 * util.EPS * 1.75 ** dim * np.abs(e).max()
            worst = max(worst, err / bound)
            assert err <= bound, ("refine", i, err, bound)
    print(f"{pattern}: worst refined patch at {worst:.3f} of its bound")


@pytest.mark.parametrize("n", [8, 16])
def test_one_slab_per_patch(n):
    """4096 patches: stencilSlabs gives one slab per patch, the instantiations a production-size level runs (k_regrid3d<N, 1>,
    k_indicator3d<N, 1>). The mixed pattern: 8 refined patches, one coarsened, the rest copied."""
    m = util.mesh("uniform", 4, 3)
    m2 = m.adapt(ru.mixed_flags(m))
    H, H2 = capi.Hierarchy(m, n), capi.Hierarchy(m2, n)
    g, g2 = capi.GMG(H), capi.GMG(H2)
    assert H.sizes(0)[0] >= 2048 and H2.sizes(0)[0] >= 2048
    u = util.rand_vec(H.cells(0), 51)
    us, ud = g.new_vector(0, u), g2.new_vector(0)
    ud.set(123.0)
    assert np.array_equal(g.patch_indicator(us), ru.indicator(u, H.sizes(0)[0], n, 3))
    capi.regrid(g, us, g2, ud)
    got = ud.download().reshape(H2.sizes(0)[0], -1)
    want, kinds = ru.regrid(H.leaf_tree(), H2.leaf_tree(), u, n, 3)
    want = want.reshape(got.shape)
    assert [(kinds == k).sum() for k in (ru.COPY, ru.REFINE, ru.COARSEN)] == [4096 - 16, 64, 1]
    exact = kinds != ru.REFINE
    assert np.array_equal(got[exact], want[exact])  # (the coarsen statement is te_restrict's bits: test_transfer, test_regrid_host.py)
    err, bound = np.abs(got[~exact] - want[~exact]).max(), 32 * util.EPS * 1.75 ** 3 * np.abs(u).max()
    print(f"n={n}: refined patches |delta| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert np.array_equal(us.download(), u)


def test_adapted_mesh_runs_the_whole_stack(case):
    n, dim = case["n"], case["dim"]
    A = adapted(case, "mixed")
    g, H = A["g"], A["H"]
    assert A["m"].is_balanced()
    levels = util.independent_levels(A["m"], H)
    u = util.rand_vec(levels[0].size, 60)
    du, df = g.new_vector(0, u), g.new_vector(0)
    g.apply(du, df)
    err, tol = np.abs(df.download() - orc.apply(levels[0], u)).max(), util.op_tol(levels[0], u)
    print(f"apply: |delta| = {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    f = util.rand_vec(levels[0].size, 61)
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)
    assert o.fuse == 3
    dv = g.new_vector(0)
    g.cycle(o, g.new_vector(0, f), dv)
    ref = orc.cycle(levels, orc.cycle_opts(smoother=capi.SMOOTH_RBGS), f)
    rel = np.abs(dv.download() - ref).max() / np.abs(ref).max()
    print(f"cycle: relative |delta| = {rel:.3e}")
    assert rel <= 1e-10
    b, x = g.new_vector(0), g.new_vector(0)
    g.init_problem(b, None, problem=capi.PROBLEM_GAUSS)
    its, rr = g.bicgstab(x, b, o, tol=1e-12)
    print(f"bicgstab (gauss): {its} iterations, relative residual {rr:.2e}")
    assert rr <= 1e-12 and its < 200


def test_vcycle_is_untouched_by_a_regrid(case):
    g, H = case["g"], case["H"]
    A = adapted(case, "+1")
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)

    def cycle_sum(gg, HH, seed):
        f, u = gg.new_vector(0, util.rand_vec(HH.cells(0), seed)), gg.new_vector(0)
        gg.cycle(o, f, u)
        return u.checksumLocal()
    before = cycle_sum(g, H, 70), cycle_sum(A["g"], A["H"], 71)
    us, ud = g.new_vector(0, util.rand_vec(H.cells(0), 72)), A["g"].new_vector(0)
    capi.regrid(g, us, A["g"], ud)
    g.patch_indicator(us)
    assert (cycle_sum(g, H, 70), cycle_sum(A["g"], A["H"], 71)) == before


def test_refusals():
    m = util.mesh("uniform", 1, 3)
    m2 = m.adapt({int(i): 1 for i in m.leaves()})
    m3 = m2.adapt({int(i): 1 for i in m2.leaves()})
    H, H2, H3, H8 = capi.Hierarchy(m, 4), capi.Hierarchy(m2, 4), capi.Hierarchy(m3, 4), capi.Hierarchy(m2, 8)
    g, g2, g3, g8 = capi.GMG(H), capi.GMG(H2), capi.GMG(H3), capi.GMG(H8)
    u = g.new_vector(0)
    capi.regrid(g, u, g2, g2.new_vector(0))
    capi.regrid(g2, g2.new_vector(0), g, u)
    capi.regrid(g, u, g, g.new_vector(0))  # the same mesh: all copies
    bad = [lambda: capi.regrid(g, u, g8, g8.new_vector(0)),  # another n
           lambda: capi.regrid(g, g.new_boundary_vector(0), g2, g2.new_vector(0)),
           lambda: capi.regrid(g, u, g2, g2.new_boundary_vector(0)),
           lambda: capi.regrid(g, u, g2, g2.new_face_vector(0)),
           lambda: capi.regrid(g, u, g2, g2.new_vector(1)),  # another level
           lambda: capi.regrid(g, g2.new_vector(0), g2, g2.new_vector(0)),  # another solver's vector
           lambda: capi.regrid(g, u, g, u),
           lambda: g.patch_indicator(g.new_boundary_vector(0)),
           lambda: g.patch_indicator(g.new_vector(0), level=1),
           lambda: g.patch_indicator(g2.new_vector(0))]
    for k, call in enumerate(bad):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL, k
    with pytest.raises(capi.TeError) as e:
        capi.regrid(g, u, g3, g3.new_vector(0))  # two adapt steps apart
    first = int(H3.leaf_tree()["id"][0])
    assert e.value.code == capi.TE_EINVAL and f"node id {first} " in str(e.value), str(e.value)
    with pytest.raises(capi.TeError) as e:
        capi.regrid(g3, g3.new_vector(0), g, u)
    assert e.value.code == capi.TE_EINVAL and "node id" in str(e.value)
    hs = capi.Hierarchy(m2, 4, rank=0, nranks=2)
    gs = capi.GMG(hs)
    for call in (lambda: capi.regrid(g, u, gs, gs.new_vector(0)), lambda: capi.regrid(gs, gs.new_vector(0), g, u)):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_ESTATE and "sharded" in str(e.value)
