"""-m gpu: the sub-patch coarse solve of the variable-coefficient path (include/te_hip.h te_gmg_set_coef_coarse)
against an ordinary solver on the split tree (bit for bit) and against the numpy statement of tests/coefcoarse_util.py, which
tests/test_coef_coarse_host.py pins on its own.

Bounds (none of them comes from what the kernels give):
  one-level hierarchies   np.array_equal: the auxiliary solver runs the kernels of an ordinary solver on the same tree on the same numbers
  cycle / solve           1e-10 relative; iteration count +-1 and 1e-8 relative: the conventions of test_gpu_varcoef.py
  what it is for          the composition gives 6 iterations against 12 (tests/test_coef_coarse_host.py); +-1 on each side leaves 4, asked 3

The incoming iterate of the coarsest level: te_vcycle sets u to zero (Cycle.h:118) and every descent sets the coarser u to zero, so on
every public route the sub-solve starts from zero whatever the caller's u held; the tests fill u with random numbers all the same. The
SECOND sub-cycle starts from the first one's result: on the comparison solver it is carried by the cycle composed from the public
per-operation entries (te_smooth, te_residual, te_restrict, te_prolong_*), which launch the cycle driver's own kernels -- the first
test below holds that composition to te_vcycle's bits before it is used."""
import functools

import numpy as np
import pytest

from pressurepoissonsolver_amd import capi
from tests import bc_util, coefcoarse_util as cu, projection_util as pu, prolong_util, reaction_util as ru, util, varcoef_util as vc
from tests.varcoef_util import masks_of, random_beta_faces as random_beta, refused, rel, solve_setup

pytestmark = pytest.mark.gpu

SUB, SWEEPS = capi.COEF_COARSE_SUBCYCLE, capi.COEF_COARSE_SWEEPS
# (dim, n, sub_n): one and two refinements of every 3D sub-patch kernel size that fits, three refinements of 4^3 patches (the Morton
# order of the offset table), 2D with two and three refinements
ONE_LEVEL = [(3, 8, 4), (3, 16, 4), (3, 32, 8), (3, 32, 4), (2, 16, 4), (2, 64, 8)]


class Composed:
    """GMG/Cycle.h:56-126 on solver g from the public per-operation entries, u CARRIED (te_vcycle zeroes it)"""

    def __init__(self, g):
        self.g = g
        self.w = [dict(r=g.new_vector(l), f=g.new_vector(l), u=g.new_vector(l)) for l in range(g.num_levels)]

    def visit(self, o, l, f, u):
        g = self.g

        def smooth(k):
            if k > 0:
                g.smooth(f, u, level=l, smoother=o.smoother, omega=o.omega, sweeps=k)

        if l == g.num_levels - 1:
            return smooth(o.coarse_sweeps)

        def descend():
            r, cf, cu_ = self.w[l]["r"], self.w[l + 1]["f"], self.w[l + 1]["u"]
            g.residual(u, f, r, level=l)
            g.restrict(cf, r, fine_level=l)
            cu_.set(0.0)
            self.visit(o, l + 1, cf, cu_)
            (g.interpolate if g.interpolator == capi.INTERP_DIRECT else g.interpolate_linear)(cu_, u, fine_level=l)

        smooth(o.pre_sweeps)
        descend()
        if o.cycle_type == 1:
            smooth(o.mid_sweeps)
            descend()
        smooth(o.post_sweeps)


@functools.lru_cache(maxsize=None)
def one_level(dim, n, s, mask):
    """g1: one patch of n^dim on the unit root; g2: an ordinary solver on the root refined log2(n / s) times with patches of s^dim"""
    m, H, levels = bc_util.setup("uniform", n, 0, mask, dim)
    assert H.num_levels == 1 and levels[0].P == 1
    sub = cu.Sub(levels[0], s)
    g1, g2 = capi.GMG(H), capi.GMG(sub.H)
    return dict(g1=g1, g2=g2, sub=sub, big=levels[0], comp=Composed(g2), H=H)


def set_both(c, beta, sigma):
    """beta (and sigma) of the big patch on g1, their split on g2"""
    g1, g2, sub = c["g1"], c["g2"], c["sub"]
    g1.set_coefficient(g1.new_face_vector(0, pu.pack(*beta)))
    g2.set_coefficient(g2.new_face_vector(0, pu.pack(*sub.split_faces(beta))))
    if sigma is not None:
        g1.set_reaction(g1.new_vector(0, sigma))
        g2.set_reaction(g2.new_vector(0, sub.split(sigma)))


def sub_solve_on_g2(c, o, f, u0, cycles):
    """the merge of `cycles` cycles of g2 on split f: te_vcycle first (it zeroes u), the others carried by the composition"""
    g2, sub = c["g2"], c["sub"]
    df, du = g2.new_vector(0, sub.split(f)), g2.new_vector(0, sub.split(u0))
    g2.cycle(o, df, du)
    for _ in range(cycles - 1):
        c["comp"].visit(o, 0, df, du)
    return sub.merge(du.download())


OPTS = [(sm, ct, cyc, ip) for sm in (capi.SMOOTH_RBGS, capi.SMOOTH_JACOBI) for ct in (0, 1) for cyc in (1, 2) for ip in (capi.INTERP_DIRECT, capi.INTERP_LINEAR)]


@pytest.mark.parametrize("with_sigma", [False, True], ids=["beta", "beta+sigma"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["dirichlet", "neumann", "mixed"])
@pytest.mark.parametrize("dim,n,s", ONE_LEVEL, ids=lambda v: str(v))
def test_one_level_hierarchies_bit_for_bit(dim, n, s, kind, with_sigma):
    c = one_level(dim, n, s, masks_of(dim)[kind])
    g1, g2, big = c["g1"], c["g2"], c["big"]
    beta = random_beta(big, 7)
    sigma = np.random.default_rng(8).uniform(0.0, 50.0, big.size) if with_sigma else None
    f, u0 = util.rand_vec(big.size, 9), util.rand_vec(big.size, 10)
    try:
        set_both(c, beta, sigma)
        for sm, ct, cycles, interp in OPTS:
            o = g1.default_opts(smoother=sm, cycle_type=ct, coarse_sweeps=3)
            g1.set_interpolator(interp)
            g2.set_interpolator(interp)
            g1.set_coef_coarse(SUB, s, cycles)
            assert g1.coef_coarse() == (SUB, s, cycles)
            if cycles == 1 and sm == capi.SMOOTH_RBGS:  # the composition that carries u: te_vcycle's bits from a zero iterate
                df, du, dv = g2.new_vector(0, c["sub"].split(f)), g2.new_vector(0), g2.new_vector(0)
                g2.cycle(o, df, du)
                c["comp"].visit(o, 0, df, dv)
                assert np.array_equal(du.download(), dv.download()), (ct, interp)
            df1, du1 = g1.new_vector(0, f), g1.new_vector(0, u0)
            g1.cycle(o, df1, du1)
            got, want = du1.download(), sub_solve_on_g2(c, o, f, u0, cycles)
            assert np.isfinite(got).all() and np.abs(got).max() > 0
            assert np.array_equal(got, want), (sm, ct, cycles, interp)
    finally:
        for g in (g1, g2):
            g.set_interpolator(capi.INTERP_DIRECT)
            g.set_coefficient(None)
        g1.set_coef_coarse(SWEEPS)


# ---- inside a hierarchy, against the CPU composition
INSIDE = [("uniform", 8, 1, 3), ("2refine.bin", 8, 0, 3), ("uniform", 16, 2, 2), ("2d2ref.bin", 16, 0, 2)]


@pytest.mark.parametrize("interp", [capi.INTERP_DIRECT, capi.INTERP_LINEAR], ids=["direct", "linear"])
@pytest.mark.parametrize("with_sigma", [False, True], ids=["beta", "beta+sigma100"])
@pytest.mark.parametrize("beta_fn", [vc.smooth_beta, vc.jump_beta], ids=["smooth", "jump"])
@pytest.mark.parametrize("name,n,div,dim", INSIDE, ids=lambda v: str(v))
def test_cycle_and_solve_against_the_cpu_composition(name, n, div, dim, beta_fn, with_sigma, interp):
    H, levels, g = solve_setup(name, n, div, dim)
    prolong = prolong_util.direct if interp == capi.INTERP_DIRECT else prolong_util.prolong_linear_add
    L = levels[0]
    beta0 = vc.beta_from(H.tables(0), n, dim, beta_fn)
    betas = vc.restrict_all(levels, beta0)
    sigmas = ru.restrict_all(levels, np.full(L.size, 100.0)) if with_sigma else None
    sub = cu.make_sub(levels, betas, sigmas, 4, 2)
    b = util.rand_vec(L.size, 5)
    g.set_interpolator(interp)
    try:
        g.set_coef_coarse(SUB, 4, 2)
        g.set_coefficient(g.new_face_vector(0, pu.pack(*beta0)))
        if with_sigma:
            g.set_reaction(g.new_vector(0, sigmas[0]))
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=8)
        db, du = g.new_vector(0, b), g.new_vector(0)
        g.cycle(o, db, du)
        err = rel(du.download(), vc.cycle(levels, betas, b, prolong, sigmas=sigmas, sub=sub, coarse=8))
        print(f"cycle: {err:.3e}")
        assert err <= 1e-10
        x_ref, its_ref = vc.bicgstab(levels, betas, b, prolong, sigmas=sigmas, sub=sub, tol=1e-10, coarse=8)
        dx = g.new_vector(0)
        its, rr = g.bicgstab(dx, db, o, tol=1e-10, max_it=40)
        print(f"solve: {its} iterations on the device, {its_ref} in the composition, relative residual {rr:.2e}")
        assert rr <= 1e-10 and abs(its - its_ref) <= 1
        assert rel(dx.download(), x_ref) <= 1e-8
    finally:
        g.set_interpolator(capi.INTERP_DIRECT)
        g.set_coefficient(None)
        g.set_coef_coarse(SWEEPS)


def test_it_does_what_it_is_for():
    """a 32^2 coarsest patch: two sub-cycles with 8 sweeps on the 4^2 patch against 16 plain sweeps"""
    H, levels, g = solve_setup("uniform", 32, 1, 2)
    beta0 = vc.beta_from(H.tables(0), 32, 2, vc.smooth_beta)
    b = g.new_vector(0, util.rand_vec(levels[0].size, 5))
    try:
        g.set_coefficient(g.new_face_vector(0, pu.pack(*beta0)))
        x = g.new_vector(0)
        its_sweeps, rr0 = g.bicgstab(x, b, g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=16), tol=1e-10, max_it=60)
        g.set_coef_coarse(SUB, 4, 2)
        x.set(0.0)
        its_sub, rr1 = g.bicgstab(x, b, g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=8), tol=1e-10, max_it=60)
        print(f"iterations: {its_sweeps} with 16 sweeps, {its_sub} with the sub-cycle (4, 2) and 8 sweeps")
        assert rr0 <= 1e-10 and rr1 <= 1e-10
        assert its_sub <= its_sweeps - 3
    finally:
        g.set_coefficient(None)
        g.set_coef_coarse(SWEEPS)


# ---- state and errors
def test_default_and_the_setting_survives_the_coefficient():
    c = one_level(3, 8, 4, 0)
    g1, g2, big = c["g1"], c["g2"], c["big"]
    f, u0 = util.rand_vec(big.size, 9), util.rand_vec(big.size, 10)
    o = g1.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=3)

    def cyc1():
        du = g1.new_vector(0, u0)
        g1.cycle(o, g1.new_vector(0, f), du)
        return du.download()

    try:
        assert g1.coef_coarse()[0] == SWEEPS
        set_both(c, random_beta(big, 7), None)
        before = cyc1()
        g1.set_coef_coarse(SWEEPS)
        assert g1.coef_coarse()[0] == SWEEPS and np.array_equal(cyc1(), before)
        g1.set_coef_coarse(SUB)  # sub_n = 0: 8 is not valid for n = 8, the smallest valid size
        assert g1.coef_coarse() == (SUB, 4, 2)
        first = cyc1()
        assert not np.array_equal(first, before)
        assert np.array_equal(first, sub_solve_on_g2(c, o, f, u0, 2))
        # cleared and set again with another beta: the setting stays, the sub-solve follows the new beta
        g1.set_coefficient(None)
        assert g1.coef_coarse() == (SUB, 4, 2) and not g1.has_coefficient()
        set_both(c, random_beta(big, 11), None)
        assert g1.coef_coarse() == (SUB, 4, 2)
        second = cyc1()
        assert not np.array_equal(second, first)
        assert np.array_equal(second, sub_solve_on_g2(c, o, f, u0, 2))
        # sigma, then a new beta: sigma is cleared in the auxiliary solver as well
        sigma = np.random.default_rng(8).uniform(0.0, 50.0, big.size)
        set_both(c, random_beta(big, 11), sigma)
        with_sigma = cyc1()
        assert not np.array_equal(with_sigma, second)
        assert np.array_equal(with_sigma, sub_solve_on_g2(c, o, f, u0, 2))
        set_both(c, random_beta(big, 11), None)
        assert not g1.has_reaction() and np.array_equal(cyc1(), second)
        # te_gmg_release_workspace: the auxiliary solver stays while the sub-cycle is selected, goes in the other kind and comes back
        g1.release_workspace()
        assert np.array_equal(cyc1(), second)
        g1.set_coef_coarse(SWEEPS)
        cyc_sweeps = cyc1()
        assert not np.array_equal(cyc_sweeps, second)
        g1.release_workspace()
        assert np.array_equal(cyc1(), cyc_sweeps)
        g1.set_coef_coarse(SUB, 4, 2)
        assert np.array_equal(cyc1(), second)
        g1.set_coef_coarse(SWEEPS)
        assert np.array_equal(cyc1(), cyc_sweeps)
    finally:
        for g in (g1, g2):
            g.set_coefficient(None)
        g1.set_coef_coarse(SWEEPS)


def test_without_a_coefficient_nothing_changes():
    m, H, levels = util.setup("2refine.bin", 8, 1)
    g = capi.GMG(H)
    f, u = g.new_vector(0, util.rand_vec(levels[0].size, 3)), g.new_vector(0)
    g.cycle(g.default_opts(), f, u)
    before = u.checksumLocal()
    g.set_coef_coarse(SUB, 4, 2)  # (no beta set: allowed)
    assert g.coef_coarse() == (SUB, 4, 2) and not g.has_coefficient()
    g.cycle(g.default_opts(), f, u)
    assert u.checksumLocal() == before
    g.set_coef_coarse(SWEEPS)
    g.cycle(g.default_opts(), f, u)
    assert u.checksumLocal() == before


def test_refusals():
    g = capi.GMG(capi.Hierarchy(capi.Mesh.unit_root(3), 32))
    for bad in (lambda: g.set_coef_coarse(7), lambda: g.set_coef_coarse(-1), lambda: g.set_coef_coarse(SUB, 4, 0), lambda: g.set_coef_coarse(SWEEPS, 0, 0),
                lambda: g.set_coef_coarse(SUB, 5), lambda: g.set_coef_coarse(SUB, 2), lambda: g.set_coef_coarse(SUB, 6), lambda: g.set_coef_coarse(SUB, 32),
                lambda: g.set_coef_coarse(SUB, -4)):
        refused(bad, capi.TE_EINVAL)
    assert g.coef_coarse() == (SWEEPS, 0, 2)  # a refused call changes nothing
    g.set_coef_coarse(SUB, 16, 3)
    assert g.coef_coarse() == (SUB, 16, 3)
    g.set_coef_coarse(SUB)
    assert g.coef_coarse() == (SUB, 8, 2)  # sub_n = 0 in 3D: 8 where valid
    g8 = capi.GMG(capi.Hierarchy(capi.Mesh.unit_root(3), 8))
    refused(lambda: g8.set_coef_coarse(SUB, 8), capi.TE_EINVAL)  # n / sub_n = 1
    g24 = capi.GMG(capi.Hierarchy(capi.Mesh.unit_root(2), 24))
    refused(lambda: g24.set_coef_coarse(SUB, 8), capi.TE_EINVAL)  # n / sub_n = 3
    g24.set_coef_coarse(SUB)
    assert g24.coef_coarse() == (SUB, 6, 2)  # 24 / 4 = 6 is no power of two: the smallest valid size
    # a truncated hierarchy: the coarsest level has eight patches
    gt = capi.GMG(capi.Hierarchy(util.mesh("uniform", 1), 8, max_levels=1))
    refused(lambda: gt.set_coef_coarse(SUB), capi.TE_EUNSUPPORTED, "8 patches")
    gt.set_coef_coarse(SWEEPS)  # the default is always accepted
    # no valid sub-patch size: n = 4 in 3D, no multiple of 4 in 2D
    refused(lambda: capi.GMG(capi.Hierarchy(capi.Mesh.unit_root(3), 4)).set_coef_coarse(SUB), capi.TE_EUNSUPPORTED, "n = 4")
    refused(lambda: capi.GMG(capi.Hierarchy(capi.Mesh.unit_root(2), 6)).set_coef_coarse(SUB), capi.TE_EUNSUPPORTED, "n = 6")
    # sharded
    gs = capi.GMG(capi.Hierarchy(util.mesh("uniform", 2), 8, rank=0, nranks=2))
    refused(lambda: gs.set_coef_coarse(SUB), capi.TE_ESTATE, "sharded")
    gs.set_coef_coarse(SWEEPS)


def test_refusals_already_in_place_stay():
    H, levels, g = solve_setup("uniform", 8, 1, 3)
    f, u, r = g.new_vector(0, util.rand_vec(levels[0].size, 1)), g.new_vector(0), g.new_vector(0)
    beta = g.new_face_vector(0)
    beta.set(1.5)
    try:
        g.set_coefficient(beta)
        g.set_coef_coarse(SUB, 4, 2)
        for call in (lambda: g.fmg(f, u, g.default_opts()), lambda: g.patch_apply(u, r), lambda: g.schur_solve(f, u, g.new_iface_vector(0))):
            refused(call, capi.TE_ESTATE, "coefficient")
        for sm in (capi.SMOOTH_PATCH_SOLVE, capi.SMOOTH_PATCH_BCGS):
            refused(lambda: g.cycle(g.default_opts(smoother=sm), f, u), capi.TE_EUNSUPPORTED)
            refused(lambda: g.smooth(f, u, smoother=sm), capi.TE_EUNSUPPORTED)
        # te_smooth on the coarsest level is untouched: one sweep of the whole patch
        lc = g.num_levels - 1
        fc, uc = g.new_vector(lc, util.rand_vec(levels[lc].size, 2)), g.new_vector(lc, util.rand_vec(levels[lc].size, 3))
        g.smooth(fc, uc, level=lc, smoother=capi.SMOOTH_RBGS)
        with_sub = uc.download()
        g.set_coef_coarse(SWEEPS)
        uc.upload(util.rand_vec(levels[lc].size, 3))
        g.smooth(fc, uc, level=lc, smoother=capi.SMOOTH_RBGS)
        assert np.array_equal(uc.download(), with_sub)
    finally:
        g.set_coefficient(None)
        g.set_coef_coarse(SWEEPS)


def test_profile_rows():
    m, H, levels = util.setup("uniform", 8, 1)
    fresh, g = capi.GMG(H), capi.GMG(H)
    f = util.rand_vec(levels[0].size, 3)
    o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=8)

    def rows_of(s, kind):
        beta = s.new_face_vector(0)
        beta.set(1.25)
        if kind is not None:
            s.set_coef_coarse(kind, 4, 2)
        s.profile(True)
        s.profile_reset()
        s.set_coefficient(beta)
        s.cycle(o, s.new_vector(0, f), s.new_vector(0))
        rows = s.profile_rows()
        s.profile(False)
        return rows

    parent = rows_of(fresh, None)  # a solver that never heard of the call: the rows of the commit before
    sub = rows_of(g, SUB)
    sweeps = rows_of(g, SWEEPS)  # (the auxiliary solver still exists)
    assert set(sweeps) == set(parent), (sorted(sweeps), sorted(parent))
    assert {k: v["calls"] for k, v in sweeps.items()} == {k: v["calls"] for k, v in parent.items()}
    assert "coef_split" not in parent and "coef_merge" not in parent
    # one cycle: f and u split in one launch, u merged in one; set_coefficient splits the coarsest beta in one more
    assert sub["coef_split"]["calls"] == 2 and sub["coef_merge"]["calls"] == 1, sub
    assert sub["coef_split"]["cells"] > 0 and sub["coef_merge"]["cells"] == 8 ** 3
    assert sub["rbgs_coef"]["calls"] > sweeps["rbgs_coef"]["calls"]
    assert sub["faces_restrict"]["calls"] > sweeps["faces_restrict"]["calls"]  # the auxiliary solver's own levels
    assert set(sub) - set(sweeps) <= {"coef_split", "coef_merge", "prolong_add", "restrict", "resid_coef", "vecop"}, sorted(sub)
