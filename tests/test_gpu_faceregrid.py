"""-m gpu: te_faces_regrid, the divergence-preserving transfer of a face vector between two meshes one te_mesh_adapt apart, against
its numpy statement (tests/faceregrid_util.py, itself checked on the CPU by tests/test_faceregrid_host.py) and against te_divergence
on both solvers.

Tolerances. Copied patches bit for bit; coarsened patches bit for bit against the statement (sums and a multiplication by a power of
two: nothing a compiler may contract); refined patches |delta| <= 32 eps (3 + sum_{b != a} h_a / h_b) M for component a, M = max|U|
over the source patch -- (3 + sum h_a / h_b) M is the largest value the rule can produce (slopes up to M at a one-sided edge,
corrections up to (h_a / h_b) M each), at most 16 roundings on each of the two sides. Divergence: faceregrid_util.div_bound, 64 eps
sum_a max|U_a| / h_a^fine."""
import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi
from tests import faceregrid_util as fu, regrid_util as ru, util

pytestmark = pytest.mark.gpu

# (mesh, n, divides, dim): the shapes of tests/test_gpu_regrid.py -- the smallest patch, a z-slab size with several blocks, the
# production patch size (64 patches of 32^3 after +1: eight slabs), trees at a four-slab size and five levels deep, the 2D kernel on a
# tree and at 64^2. One slab per patch: the rule gives it from 2048 patches on (test_one_slab_per_patch below); on few patches TE_ZS_PIN
# gives it and every other admitted count (tests/test_gpu_slab_matrix.py).
SHAPES = [("uniform", 4, 2, 3), ("uniform", 8, 2, 3), ("uniform", 32, 1, 3), ("2refine.bin", 16, 0, 3), ("multi_refine.bin", 8, 0, 3),
          ("2d2ref.bin", 4, 0, 2), ("uniform", 64, 2, 2)]
IDS = lambda c: f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}d"  # noqa: E731
_cases = {}


def get_case(shape):
    if shape not in _cases:
        name, n, div, dim = shape
        orc.set_threads(16)
        m = util.mesh(name, div, dim)
        H = capi.Hierarchy(m, n)
        _cases[shape] = dict(name=name, n=n, dim=dim, m=m, H=H, g=capi.GMG(H), adapted={})
    return _cases[shape]


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request):
    return get_case(request.param)


def flags(m, pattern):
    if pattern != "mixed":
        return {int(i): int(pattern) for i in m.leaves()}
    return {int(m.leaves()[0]): 1} if len(m.leaves()) == 1 << m.dim else ru.mixed_flags(m)  # (a one-family mesh: +1 on one leaf)


def adapted(case, pattern):
    if pattern not in case["adapted"]:
        m2 = case["m"].adapt(flags(case["m"], pattern))
        H2 = capi.Hierarchy(m2, case["n"])
        case["adapted"][pattern] = dict(m=m2, H=H2, g=capi.GMG(H2))
    return case["adapted"][pattern]


def spacings(H):
    return H.tables(0)["lengths"] / H.n


def random_faces(H, seed):
    return util.rand_vec(H.sizes(0)[0] * capi.face_vector_size(H.n, H.dim), seed)


def single_valued(H, U):
    """U with the upper patch's plane 0 set to the lower patch's HI block on every same-level shared face, as a velocity on a mesh is:
    only then is a coarse cell's divergence the mean of its children's (the mid-plane is taken from the upper child alone)"""
    lo, hi = capi.face_vector_views(U, H.n, H.dim)
    for p, a, q in same_level_pairs(H):
        sl = [slice(None)] * H.dim
        sl[H.dim - 1 - a] = 0
        lo[q, a][tuple(sl)] = hi[p, a].reshape((H.n,) * (H.dim - 1))
    return U


def destination(A, fill=123.0):
    return A["g"].new_face_vector(0, np.full(A["H"].sizes(0)[0] * capi.face_vector_size(A["H"].n, A["H"].dim), fill))


def check_against_statement(H, H2, U, got, label):
    """-> kinds. got: the destination face vector (host); every patch is compared with the statement by the rule of its kind"""
    n, dim = H.n, H.dim
    hs = spacings(H)
    want, kinds = fu.regrid_faces(H.leaf_tree(), H2.leaf_tree(), U, n, dim, hs)
    glo, ghi = capi.face_vector_views(got, n, dim)
    wlo, whi = capi.face_vector_views(want, n, dim)
    ulo, uhi = capi.face_vector_views(U, n, dim)
    src_leaf = {int(i): p for p, i in enumerate(H.leaf_tree()["id"])}
    dst = H2.leaf_tree()
    exact = kinds != fu.REFINE
    assert np.array_equal(glo[exact], wlo[exact]) and np.array_equal(ghi[exact], whi[exact]), label  # copy, coarsen: bit for bit
    worst = 0.0
    for p in np.flatnonzero(~exact):
        q = src_leaf[int(dst["tree_parent"][p])]
        M = max(np.abs(ulo[q]).max(), np.abs(uhi[q]).max())
        for a in range(dim):
            err = max(np.abs(glo[p, a] - wlo[p, a]).max(), np.abs(ghi[p, a] - whi[p, a]).max())
            bound = 32 * util.EPS * (3 + sum(hs[q, a] / hs[q, b] for b in range(dim) if b != a)) * M
            worst = max(worst, err / bound)
            assert err <= bound, (label, "refine", int(dst["id"][p]), a, err, bound)
    print(f"{label}: copy {(kinds == fu.COPY).sum()} refine {(kinds == fu.REFINE).sum()} coarsen {(kinds == fu.COARSEN).sum()}; "
          f"worst refined component at {worst:.3f} of its bound")
    return kinds


@pytest.mark.parametrize("pattern", ["+1", "-1", "mixed"])
def test_transfer_against_the_statement(case, pattern):
    g, H, dim = case["g"], case["H"], case["dim"]
    A = adapted(case, pattern)
    U = random_faces(H, 80)
    Us, Ud = g.new_face_vector(0, U), destination(A)
    A["g"].profile(True)
    A["g"].profile_reset()
    capi.regrid_faces(g, Us, A["g"], Ud)
    rows = A["g"].profile_rows()
    A["g"].profile(False)
    # the transfer is one launch of k_facexfer*, on the destination solver, over its cells -- and nothing else ran
    assert {k: (v["calls"], v["cells"]) for k, v in rows.items() if v["calls"]} == {"regrid_faces": (1, A["H"].cells(0))}, rows
    kinds = check_against_statement(H, A["H"], U, Ud.download(), pattern)
    assert np.array_equal(Us.download(), U)
    if pattern == "mixed" and case["name"] == "uniform" and len(case["m"].leaves()) > 1 << dim:
        assert all((kinds == k).any() for k in (fu.COPY, fu.REFINE, fu.COARSEN))
    if pattern == "+1":
        assert (kinds == fu.REFINE).all()
    if pattern == "-1" and case["name"] == "uniform":
        assert (kinds == fu.COARSEN).all()


@pytest.mark.parametrize("pattern", ["+1", "-1", "mixed"])
def test_divergence_commutes_on_the_device(case, pattern):
    g, H, n, dim = case["g"], case["H"], case["n"], case["dim"]
    A = adapted(case, pattern)
    U = single_valued(H, random_faces(H, 81))
    Us, Ud = g.new_face_vector(0, U), destination(A)
    capi.regrid_faces(g, Us, A["g"], Ud)
    ds, dd = g.new_vector(0), A["g"].new_vector(0)
    g.divergence(Us, ds)
    A["g"].divergence(Ud, dd)
    shape = (-1,) + (n,) * dim
    src_div, dst_div = ds.download().reshape(shape), dd.download().reshape(shape)
    restricted = [ds]  # te_restrict of the source divergence: the mean over the children, on the device
    for l in range(H.num_levels - 1):
        restricted.append(g.new_vector(l + 1))
        g.restrict(restricted[l + 1], restricted[l], fine_level=l)
    level_ids = [H.tables(l)["id"] for l in range(H.num_levels)]
    src, dst, hs = H.leaf_tree(), A["H"].leaf_tree(), spacings(H)
    src_leaf = {int(i): p for p, i in enumerate(src["id"])}
    ulo, uhi = capi.face_vector_views(U, n, dim)
    bound_of = lambda q, hf: fu.div_bound(fu.patch_faces(ulo[q], uhi[q], n, dim), hf)  # noqa: E731
    worst = 0.0
    for p, (i, par, o) in enumerate(zip(dst["id"], dst["tree_parent"], dst["orthant"])):
        if int(i) in src_leaf:
            assert np.array_equal(dst_div[p], src_div[src_leaf[int(i)]]), ("copy", int(i))
        elif int(par) in src_leaf:
            q = src_leaf[int(par)]
            err, bound = np.abs(dst_div[p] - fu.parent_cells(src_div[q], int(o), n, dim)).max(), bound_of(q, hs[q] / 2)
            worst = max(worst, err / bound)
            assert err <= bound, ("refine", int(i), err, bound)
        else:
            kids = [int(q) for q in np.flatnonzero(src["tree_parent"] == i)]
            bound = max(bound_of(q, hs[q]) for q in kids)
            l = next((l for l in range(1, H.num_levels) if int(i) in level_ids[l]), None)
            if l is not None:
                mean = restricted[l].download_patches(int(np.flatnonzero(level_ids[l] == i)[0]), 1).reshape((n,) * dim)
            else:
                mean = fu.children_mean([src_div[q] for q in sorted(kids, key=lambda q: src["orthant"][q])], dim)
            err = np.abs(dst_div[p] - mean).max()
            worst = max(worst, err / bound)
            assert err <= bound, ("coarsen", int(i), err, bound)
    print(f"{pattern}: worst patch at {worst:.3f} of its divergence bound")


def same_level_pairs(H):
    """(p, a, q): patch q is the same-level neighbour of patch p on its upper a-face"""
    t = H.tables(0)
    return [(p, a, int(t["nbr"][p, 2 * a + 1, 0])) for p in range(H.sizes(0)[0]) for a in range(H.dim) if t["nbr_kind"][p, 2 * a + 1] == 1]


def lower_plane(lo_qa, dim, a):
    return np.take(lo_qa, 0, axis=dim - 1 - a).ravel()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == "uniform"], ids=IDS)
def test_shared_faces_get_the_same_bits_in_both_copies(shape):
    case = get_case(shape)
    g, H, n, dim = case["g"], case["H"], case["n"], case["dim"]
    A = adapted(case, "+1")
    U = single_valued(H, random_faces(H, 82))
    Ud = destination(A)
    capi.regrid_faces(g, g.new_face_vector(0, U), A["g"], Ud)
    lo, hi = capi.face_vector_views(Ud.download(), n, dim)
    pairs = same_level_pairs(A["H"])
    assert len(pairs) > len(same_level_pairs(H))
    for p, a, q in pairs:
        assert np.array_equal(hi[p, a], lower_plane(lo[q, a], dim, a)), (p, a, q)


def test_projected_velocity_stays_divergence_free_across_a_regrid():
    case = get_case(("uniform", 8, 2, 3))
    g, H, n, dim = case["g"], case["H"], case["n"], case["dim"]
    A = adapted(case, "+1")
    U = g.new_face_vector(0, random_faces(H, 83))
    f, p, d = g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.divergence(U, f)
    its, rr = g.bicgstab(p, f, g.default_opts(), tol=1e-10)
    assert rr <= 1e-10
    g.project(U, p)
    g.divergence(U, d)
    before = d.infNorm()
    assert before <= 1e-6 * f.infNorm()  # the solve went as far as asked: the field is divergence-free to that
    Ud, dd = destination(A), A["g"].new_vector(0)
    capi.regrid_faces(g, U, A["g"], Ud)
    A["g"].divergence(Ud, dd)
    lo, hi = capi.face_vector_views(U.download(), n, dim)
    hs = spacings(H)
    bound = max(fu.div_bound(fu.patch_faces(lo[q], hi[q], n, dim), hs[q] / 2) for q in range(H.sizes(0)[0]))
    print(f"{its} iterations: max|div U*| {f.infNorm():.3e} -> max|div U| {before:.3e} -> on the refined mesh {dd.infNorm():.3e} (+ bound {bound:.3e})")
    assert dd.infNorm() <= before + bound


@pytest.mark.parametrize("n", [8, 16])
def test_one_slab_per_patch(n):
    """4096 patches: stencilSlabs gives one slab per patch, the instantiations a production-size level runs (k_facexfer3d<N, 1>). The
    mixed pattern: 64 refined patches, one coarsened, the rest copied."""
    m = util.mesh("uniform", 4, 3)
    m2 = m.adapt(ru.mixed_flags(m))
    H, H2 = capi.Hierarchy(m, n), capi.Hierarchy(m2, n)
    g, g2 = capi.GMG(H), capi.GMG(H2)
    assert H.sizes(0)[0] >= 2048 and H2.sizes(0)[0] >= 2048
    U = random_faces(H, 84)
    Us, Ud = g.new_face_vector(0, U), destination(dict(g=g2, H=H2))
    capi.regrid_faces(g, Us, g2, Ud)
    kinds = check_against_statement(H, H2, U, Ud.download(), f"n={n}")
    assert [(kinds == k).sum() for k in (fu.COPY, fu.REFINE, fu.COARSEN)] == [4096 - 16, 64, 1]
    assert Us.checksumLocal() == int(U.view(np.uint64).sum(dtype=np.uint64))  # the source is unchanged


def test_refusals():
    m = util.mesh("uniform", 1, 3)
    m2 = m.adapt({int(i): 1 for i in m.leaves()})
    m3 = m2.adapt({int(i): 1 for i in m2.leaves()})
    H, H2, H3, H8 = capi.Hierarchy(m, 4), capi.Hierarchy(m2, 4), capi.Hierarchy(m3, 4), capi.Hierarchy(m2, 8)
    g, g2, g3, g8 = capi.GMG(H), capi.GMG(H2), capi.GMG(H3), capi.GMG(H8)
    gd = capi.GMG(capi.Hierarchy(util.mesh("uniform", 1, 2), 4))  # a 2D solver with the same n
    null = type("Null", (), dict(h=None))()  # what the binding passes as a NULL handle
    U = g.new_face_vector(0)
    capi.regrid_faces(g, U, g2, g2.new_face_vector(0))
    capi.regrid_faces(g2, g2.new_face_vector(0), g, U)
    capi.regrid_faces(g, U, g, g.new_face_vector(0))  # the same mesh: all copies
    bad = [lambda: capi.regrid_faces(g, U, g8, g8.new_face_vector(0)),  # another n
           lambda: capi.regrid_faces(g, g.new_vector(0), g2, g2.new_face_vector(0)),  # a domain vector in either place
           lambda: capi.regrid_faces(g, U, g2, g2.new_vector(0)),
           lambda: capi.regrid_faces(g, g.new_boundary_vector(0), g2, g2.new_face_vector(0)),
           lambda: capi.regrid_faces(g, U, g2, g2.new_boundary_vector(0)),
           lambda: capi.regrid_faces(g, U, g2, g2.new_face_vector(1)),  # another level
           lambda: capi.regrid_faces(g2, g2.new_face_vector(1), g, U),
           lambda: capi.regrid_faces(g, g2.new_face_vector(0), g2, g2.new_face_vector(0)),  # another solver's vector
           lambda: capi.regrid_faces(g, U, g, U),  # the same vector
           lambda: capi.regrid_faces(g, g.new_iface_vector(0), g2, g2.new_face_vector(0)),  # an interface vector in either place
           lambda: capi.regrid_faces(g, U, g2, g2.new_iface_vector(0)),
           lambda: capi.regrid_faces(g, U, gd, gd.new_face_vector(0)),  # another dim
           lambda: capi.regrid_faces(null, U, g2, g2.new_face_vector(0)),  # NULL, each argument
           lambda: capi.regrid_faces(g, null, g2, g2.new_face_vector(0)),
           lambda: capi.regrid_faces(g, U, null, g2.new_face_vector(0)),
           lambda: capi.regrid_faces(g, U, g2, null)]
    for k, call in enumerate(bad):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL, k
    with pytest.raises(capi.TeError) as e:
        capi.regrid_faces(g, U, g3, g3.new_face_vector(0))  # two adapt steps apart
    first = int(H3.leaf_tree()["id"][0])
    assert e.value.code == capi.TE_EINVAL and f"te_faces_regrid: destination leaf with node id {first} " in str(e.value), str(e.value)
    with pytest.raises(capi.TeError) as e:
        capi.regrid_faces(g3, g3.new_face_vector(0), g, U)
    assert e.value.code == capi.TE_EINVAL and "node id" in str(e.value)
    hs = capi.Hierarchy(m2, 4, rank=0, nranks=2)
    gs = capi.GMG(hs)
    for call in (lambda: capi.regrid_faces(g, U, gs, gs.new_face_vector(0)), lambda: capi.regrid_faces(gs, gs.new_face_vector(0), g, U)):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_ESTATE and "sharded" in str(e.value)


def test_cycles_and_cell_transfers_are_untouched(case):
    g, H = case["g"], case["H"]
    A = adapted(case, "mixed")
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)
    assert o.fuse == 3

    def cycle_sum(gg, HH, seed):
        f, u = gg.new_vector(0, util.rand_vec(HH.cells(0), seed)), gg.new_vector(0)
        gg.cycle(o, f, u)
        return u.checksumLocal()

    def cells(src, dst, us):
        ud = dst.new_vector(0)
        capi.regrid(src, us, dst, ud)
        return ud.download()
    us, us2 = g.new_vector(0, util.rand_vec(H.cells(0), 90)), A["g"].new_vector(0, util.rand_vec(A["H"].cells(0), 91))
    Us, Us2 = g.new_face_vector(0, random_faces(H, 92)), A["g"].new_face_vector(0, random_faces(A["H"], 93))
    before = cycle_sum(g, H, 94), cycle_sum(A["g"], A["H"], 95)
    there, back = cells(g, A["g"], us), cells(A["g"], g, us2)
    Ud, Ud2 = destination(A), destination(case)
    capi.regrid_faces(g, Us, A["g"], Ud)  # the two calls share the destination solver's map buffer
    assert np.array_equal(cells(A["g"], g, us2), back)
    capi.regrid_faces(A["g"], Us2, g, Ud2)
    assert np.array_equal(cells(g, A["g"], us), there)
    first = Ud.download()
    capi.regrid_faces(g, Us, A["g"], Ud)
    assert np.array_equal(Ud.download(), first)
    assert (cycle_sum(g, H, 94), cycle_sum(A["g"], A["H"], 95)) == before
