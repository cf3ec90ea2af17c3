"""-m gpu: the full-multigrid solve te_fmg and its two kernels -- the quadratic FMG interpolation te_prolong_quadratic and the
restriction of boundary vectors te_boundary_restrict -- against their numpy statements (tests/fmg_util.py; the statements
themselves are checked on the CPU by tests/test_fmg_host.py) and against FMG composed from the oracle's pieces.

Tolerances. Interpolation: |delta| <= 32 eps * 40 * max|e| -- an extrapolated ghost is at most 7 max|e|, a corner at most 3 * 7 + 2,
and the weights' absolute sum is (38 / 32)^3; copy-through patches bit for bit. Boundary restriction: 4 eps * max|g| (three
additions and one exact scaling). Driver: 1e-9 * max|want| -- at most eight cycles (two per level, five levels), each held to the
project's 1e-10 cycle tolerance, the other steps at rounding. Accuracy: the cap 0.3 of DESIGN.md section 15 on |u_fmg - u_h| / |u_h - u_exact|."""
import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi, dist as tedist
from tests import bc_util, fmg_util as fu, projection_util as pju, prolong_util as pu, util

pytestmark = pytest.mark.gpu

ALL = {2: 0b1111, 3: 0b111111}
# (mesh, n, divides, dim), the shapes of tests/test_gpu_prolong_linear.py: uniform levels with one and several blocks per level and
# the production instantiation (32^3, 8 patches), coarse/fine faces and copy-through patches at the smallest and a z-slab patch size,
# a five-level tree, the 2D kernel
SHAPES = [("uniform", 4, 2, 3), ("uniform", 8, 2, 3), ("uniform", 32, 1, 3), ("2refine.bin", 4, 0, 3), ("2refine.bin", 16, 0, 3),
          ("multi_refine.bin", 8, 0, 3), ("2d2ref.bin", 4, 0, 2), ("2d2ref.bin", 16, 0, 2), ("uniform", 64, 2, 2)]
CASES = [s + (mask,) for s in SHAPES for mask in ((0, ALL[3]) + bc_util.MASKS3 if s[3] == 3 else (0, ALL[2]) + bc_util.MASKS2)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}d-{c[4]:06b}")
def case(request):
    name, n, div, dim, mask = request.param
    orc.set_threads(16)
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    return dict(H=H, levels=levels, g=capi.GMG(H), name=name, singular=mask == ALL[dim])


def test_prolong_quadratic_per_level_pair(case):
    """random coarse, fine pre-filled with 123.0: fine is SET; a patch that copies through receives exactly coarse"""
    g, levels = case["g"], case["levels"]
    copies = 0
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        e = util.rand_vec(C.size, 60 + l)
        de, du = g.new_vector(l + 1, e), g.new_vector(l)
        du.set(123.0)
        g.interpolate_quadratic(de, du, fine_level=l)
        got, want = du.download(), fu.prolong_quadratic(F, C, e)
        err, bound = np.abs(got - want).max(), 32 * util.EPS * 40 * np.abs(e).max()
        print(f"level {l}: |delta| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, l
        assert np.array_equal(de.download(), e)
        thru = np.flatnonzero(F.a["orth_on_parent"] < 0)
        copies += len(thru)
        for pf in thru:
            assert np.array_equal(got.reshape(F.P, -1)[pf], e.reshape(C.P, -1)[F.a["parent"][pf]]), (l, pf)
    if case["name"] != "uniform":
        assert copies > 0


def test_boundary_restrict_per_level_pair(case):
    g, levels = case["g"], case["levels"]
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        nf = F.nf
        b = util.rand_vec(pju.num_bfaces(F) * nf, 90 + l)
        db, dc = g.new_boundary_vector(l, b), g.new_boundary_vector(l + 1)
        g.boundary_restrict(db, dc, fine_level=l)
        got, want = dc.download(), fu.boundary_restrict(F, C, b)
        err = np.abs(got - want).max(initial=0.0)
        print(f"level {l}: |delta| = {err:.3e}")
        assert err <= 4 * util.EPS * np.abs(b).max(initial=0.0), l
        assert np.array_equal(db.download(), b)
        fi, ci = pju.bface_index(F.a["nbr_kind"]), pju.bface_index(C.a["nbr_kind"])
        for pf in np.flatnonzero(F.a["orth_on_parent"] < 0):
            for s in np.flatnonzero(fi[pf] >= 0):
                assert np.array_equal(got.reshape(-1, nf)[ci[F.a["parent"][pf], s]], b.reshape(-1, nf)[fi[pf, s]]), (l, pf, s)


# (cycles, smoother, interpolator, cycle type)
R, J, B, LIN, DIR = capi.SMOOTH_RBGS, capi.SMOOTH_JACOBI, capi.SMOOTH_PATCH_SOLVE, capi.INTERP_LINEAR, capi.INTERP_DIRECT
DRIVER = [(0, R, LIN, 0), (1, R, LIN, 0), (2, R, LIN, 0), (2, J, LIN, 0), (2, B, LIN, 0), (2, R, DIR, 0), (1, B, DIR, 0), (1, R, LIN, 1)]


@pytest.mark.parametrize("cycles,smoother,interp,ctype", DRIVER, ids=lambda v: str(v))
def test_fmg_against_the_composition(case, cycles, smoother, interp, ctype):
    g, levels = case["g"], case["levels"]
    f = util.rand_vec(levels[0].size, 70)
    bd = util.rand_vec(pju.num_bfaces(levels[0]) * levels[0].nf, 71)
    o = g.default_opts(smoother=smoother, cycle_type=ctype)
    want = fu.fmg(levels, f, bd, cycles=cycles, prolong=pu.prolong_linear_add if interp == LIN else pu.direct, smoother=smoother, pre=o.pre_sweeps,
                  post=o.post_sweeps, coarse=o.coarse_sweeps, mid=o.mid_sweeps, cycle_type=ctype, omega=o.omega, exact_coarse=o.exact_coarse)
    if case["singular"]:
        want = want - want.mean()
    g.set_interpolator(interp)
    sums = {}
    try:
        for fuse in (0, 1, 2, 3):
            o.fuse = fuse
            df, db, du = g.new_vector(0, f), g.new_boundary_vector(0, bd), g.new_vector(0)
            du.set(123.0)
            g.fmg(df, du, o, bdata=db, cycles=cycles)
            got = du.download()
            sums[fuse] = du.checksumLocal()
            if case["singular"]:
                got = got - got.mean()
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"fuse={fuse}: relative |delta| = {err:.3e}")
            assert err <= 1e-9, (fuse, err)
            assert np.array_equal(df.download(), f) and np.array_equal(db.download(), bd)
    finally:
        g.set_interpolator(DIR)
    assert sums[1] == sums[0] and sums[3] == sums[2], sums


def test_homogeneous_data_is_a_null_boundary_vector(case):
    g, levels = case["g"], case["levels"]
    f = util.rand_vec(levels[0].size, 72)
    o = g.default_opts(smoother=R)
    a, b = g.new_vector(0), g.new_vector(0)
    g.fmg(g.new_vector(0, f), a, o, bdata=None, cycles=1)
    g.fmg(g.new_vector(0, f), b, o, bdata=g.new_boundary_vector(0), cycles=1)
    x, y = a.download(), b.download()
    assert np.isfinite(x).all() and np.abs(x - y).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("name,n,div", [("uniform", 8, 2), ("uniform", 16, 2), ("2refine.bin", 8, 0)], ids=lambda v: str(v))
def test_accuracy_on_the_device(name, n, div):
    """the trig problem with exact face data, V(1,1) with RB-GS, the linear interpolator, two cycles per level"""
    m, H, levels = bc_util.setup(name, n, div, 0, 3)
    f, bd, exact = fu.trig_problem(H, 0)
    g = capi.GMG(H)
    g.set_interpolator(LIN)
    o = g.default_opts(smoother=R)
    df, db, u, uh = g.new_vector(0, f), g.new_boundary_vector(0, bd), g.new_vector(0), g.new_vector(0)
    rr = g.fmg(df, u, o, bdata=db, cycles=2)
    F0 = g.new_vector(0, f)
    g.add_boundary_rhs(db, F0)
    its, _ = g.bicgstab(uh, F0, o, tol=1e-12)
    a, b = u.download(), uh.download()
    ratio = np.linalg.norm(a - b) / np.linalg.norm(b - exact)
    r = g.new_vector(0)
    again = np.sqrt(g.residual_norm_sq(u, F0, r)) / F0.twoNorm()
    print(f"{name} n={n}: |u_fmg - u_h| / |u_h - u_exact| = {ratio:.3f}; |u_fmg - u_exact| / |u_h - u_exact| = "
          f"{np.linalg.norm(a - exact) / np.linalg.norm(b - exact):.3f}; rel_resid {rr:.3e} (recomputed {again:.3e}); the solve took {its} iterations")
    assert ratio <= 0.3
    assert abs(rr - again) <= 1e-10 * again


def profiled(g, call):
    g.profile(True)
    g.profile_reset()
    out = call()
    rows = g.profile_rows()
    g.profile(False)
    return out, {k for k, v in rows.items() if v["calls"] > 0}


@pytest.mark.parametrize("name,n,div,dim", [("uniform", 4, 3, 3), ("2refine.bin", 4, 1, 3), ("uniform", 8, 3, 2)], ids=lambda v: str(v))
def test_solver_state_is_left_as_found(name, n, div, dim):
    H = capi.Hierarchy(util.mesh(name, div, dim), n)
    g = capi.GMG(H)
    f = util.rand_vec(H.cells(0), 73)
    bd = util.rand_vec(g.new_boundary_vector(0).size, 74)
    o = g.default_opts(smoother=R, fuse=3)

    def vcycle():
        du = g.new_vector(0)
        g.cycle(o, g.new_vector(0, f), du)
        return du.checksumLocal()

    def fmg():
        du = g.new_vector(0)
        g.fmg(g.new_vector(0, f), du, o, bdata=g.new_boundary_vector(0, bd), cycles=2)
        return du.checksumLocal()

    for kind in (DIR, LIN):
        g.set_interpolator(kind)
        before, ran_before = profiled(g, vcycle)
        first, ran_fmg = profiled(g, fmg)
        assert g.interpolator == kind
        after, ran_after = profiled(g, vcycle)
        assert (after, ran_after) == (before, ran_before), (sorted(ran_after), sorted(ran_before))
        assert {"prolong_quadratic", "boundary_restrict"} <= ran_fmg, sorted(ran_fmg)
        assert not ({"prolong_quadratic", "boundary_restrict"} & ran_before)
        assert fmg() == first  # the kept work vectors
        g.release_workspace()
        assert fmg() == first  # ... and new ones
    g.set_interpolator(DIR)


def test_bad_arguments():
    H = capi.Hierarchy(util.mesh("2refine.bin"), 4)
    g, other = capi.GMG(H), capi.GMG(H)
    o = g.default_opts(smoother=R)
    fine, coarse, f = g.new_vector(0), g.new_vector(1), g.new_vector(0)
    bf, bc = g.new_boundary_vector(0), g.new_boundary_vector(1)
    last = H.num_levels - 1
    bad = [lambda: g.interpolate_quadratic(fine, coarse, fine_level=0),  # swapped
           lambda: g.interpolate_quadratic(g.new_iface_vector(1), fine, fine_level=0),
           lambda: g.interpolate_quadratic(coarse, bf, fine_level=0),
           lambda: g.interpolate_quadratic(coarse, g.new_face_vector(0), fine_level=0),
           lambda: g.interpolate_quadratic(other.new_vector(1), fine, fine_level=0),
           lambda: g.interpolate_quadratic(g.new_vector(last), g.new_vector(last), fine_level=last),
           lambda: g.boundary_restrict(bc, bf, fine_level=0),  # swapped
           lambda: g.boundary_restrict(fine, bc, fine_level=0),
           lambda: g.boundary_restrict(bf, coarse, fine_level=0),
           lambda: g.boundary_restrict(other.new_boundary_vector(0), bc, fine_level=0),
           lambda: g.boundary_restrict(g.new_boundary_vector(last), g.new_boundary_vector(last), fine_level=last),
           lambda: g.fmg(f, fine, o, cycles=-1),
           lambda: g.fmg(coarse, fine, o),
           lambda: g.fmg(f, coarse, o),
           lambda: g.fmg(f, fine, o, bdata=bc),
           lambda: g.fmg(f, fine, o, bdata=g.new_vector(0)),
           lambda: g.fmg(bf, fine, o),
           lambda: g.fmg(f, g.new_face_vector(0), o),
           lambda: g.fmg(other.new_vector(0), fine, o),
           lambda: g.fmg(f, fine, o, bdata=other.new_boundary_vector(0))]
    for i, call in enumerate(bad):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL, i
    g.interpolate_quadratic(coarse, fine, fine_level=0)
    g.boundary_restrict(bf, bc, fine_level=0)
    g.fmg(f, fine, o, bdata=bf)


def test_a_coarsest_level_of_several_patches_is_refused():
    H = capi.Hierarchy(util.mesh("uniform", 2), 8, max_levels=2)
    g = capi.GMG(H)
    with pytest.raises(capi.TeError) as e:
        g.fmg(g.new_vector(0), g.new_vector(0), g.default_opts(smoother=R))
    assert e.value.code == capi.TE_ESTATE and "max_levels" in str(e.value)


def test_sharded_hierarchy_is_refused_and_direct_still_runs():
    mesh, n = util.mesh("uniform", 2), 8
    fab = tedist.LocalFabric(2)
    hs = [capi.Hierarchy(mesh, n, rank=r, nranks=2) for r in range(2)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)

    def run(r):
        g = gs[r]
        o = g.default_opts(smoother=R)
        codes = []
        for call in (lambda: g.fmg(g.new_vector(0), g.new_vector(0), o), lambda: g.interpolate_quadratic(g.new_vector(1), g.new_vector(0), fine_level=0),
                     lambda: g.boundary_restrict(g.new_boundary_vector(0), g.new_boundary_vector(1), fine_level=0)):
            with pytest.raises(capi.TeError) as e:
                call()
            codes.append((e.value.code, str(e.value)))
        f, u = g.new_vector(0, util.rand_vec(hs[r].sizes(0)[0] * n ** 3, 5 + r)), g.new_vector(0)
        g.cycle(o, f, u)
        return codes, g.interpolator, np.isfinite(u.download()).all() and np.abs(u.download()).max() > 0

    for codes, kind, ok in fab.run(run):
        assert [c for c, _ in codes] == [capi.TE_ESTATE] * 3, codes
        assert all("sharded" in msg for _, msg in codes), codes
        assert kind == DIR and ok
