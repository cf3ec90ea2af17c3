"""-m gpu: the variable-coefficient operator div(beta grad u) (include/te_hip.h te_gmg_set_coefficient and what follows it) against
the numpy statement of tests/varcoef_util.py, which tests/test_varcoef_host.py pins to the oracle.

Bounds (none of them comes from what the kernels give):
  apply / residual   max(beta) * util.op_tol(u): a few ulps of sum |coef| |u|, every coefficient scaled by at most max(beta);
                     the same against the device composition te_divergence(1, beta (.) te_gradient(u))
  residual norm      1e-13 relative against numpy's sum over the downloaded residual (another summation order)
  one sweep          1e-11 relative 2-norm, the project's sweep figure (test_gpu_parity.py)
  beta = 2           the scaling is exact, only association differs: the project's cycle figure, 1e-10 relative 2-norm
  restriction        4 eps max|beta| (two additions and a multiplication by a power of two per entry); copy-through bit for bit
  cycle / solve      1e-10 relative; iteration count +-1 and 1e-8 relative: the conventions of test_gpu_parity.py
  end to end         max|div U| <= max|f - A_b p| + 2 max(beta) op_tol(p) + 4 eps (2 dim / h_min) max|U*|"""
import numpy as np
import pytest

from pressurepoissonsolver_amd import capi
from tests import bc_util, projection_util as pu, prolong_util, util, varcoef_util as vc
from tests.varcoef_util import CASES, SOLVES, device_betas, random_beta, refused, rel, solve_setup

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-d{c[1]}-n{c[2]}-{c[3]}d-{c[4]:06b}")
def case(request):
    name, div, n, dim, mask = request.param
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    g = capi.GMG(H)
    beta0 = random_beta(levels[0].P * pu.face_size(n, dim), 7)
    g.set_coefficient(g.new_face_vector(0, beta0))  # (the caller's vector goes away: the solver has its copy)
    assert g.has_coefficient()
    return dict(H=H, levels=levels, g=g, n=n, dim=dim, mask=mask, beta0=beta0, betas=device_betas(g, levels, n, dim))


def test_apply_and_residual(case):
    g, n, dim = case["g"], case["n"], case["dim"]
    for l, L in enumerate(case["levels"]):
        beta = case["betas"][l]
        u, f = util.rand_vec(L.size, 100 + l), util.rand_vec(L.size, 110 + l)
        du, df, dA, dr = g.new_vector(l, u), g.new_vector(l, f), g.new_vector(l), g.new_vector(l)
        g.apply(du, dA, level=l)
        A, want = dA.download(), vc.apply(L, beta, u)
        tol = max(beta[0].max(), beta[1].max()) * util.op_tol(L, u)
        err = np.abs(A - want).max()
        print(f"apply level {l}: {err / tol:.3f} of the bound")
        assert err <= tol, l
        # the device composition: div(beta (.) grad u)
        dG, db, dc = g.new_face_vector(l), g.new_face_vector(l, pu.pack(*beta)), g.new_vector(l)
        g.gradient(du, dG, level=l)
        dG.multiply(db)
        g.divergence(dG, dc, level=l)
        err = np.abs(A - dc.download()).max()
        print(f"apply against the composition, level {l}: {err / tol:.3f} of the bound")
        assert err <= tol, l
        g.residual(du, df, dr, level=l)
        r = dr.download()
        err = np.abs(r - (f - want)).max()
        print(f"residual level {l}: {err / tol:.3f} of the bound")
        assert err <= tol, l
        nsq = g.residual_norm_sq(du, df, dr, level=l)
        assert np.array_equal(dr.download(), r)
        assert abs(nsq - np.sum(r * r)) <= 1e-13 * np.sum(r * r), l


def test_one_sweep(case):
    g = case["g"]
    omega = 6.0 / 7.0
    for l, L in enumerate(case["levels"]):
        beta = case["betas"][l]
        u, f = util.rand_vec(L.size, 120 + l), util.rand_vec(L.size, 130 + l)
        for sm, want in ((capi.SMOOTH_RBGS, vc.rbgs(L, beta, f, u)), (capi.SMOOTH_JACOBI, vc.jacobi(L, beta, f, u, omega))):
            du, df = g.new_vector(l, u), g.new_vector(l, f)
            g.smooth(df, du, level=l, smoother=sm, omega=omega)
            err = rel(du.download(), want)
            print(f"sweep {sm} level {l}: {err:.3e}")
            assert err <= 1e-11, (l, sm)


def test_sweep_above_the_lds_limit():
    """2D patches of 128^2 do not fit the LDS form (n <= 64): the two colour launches k_coef_rbgs2d<0 / 1>"""
    n, dim = 128, 2
    m, H, levels = bc_util.setup("2d2ref.bin", n, 0, bc_util.MASKS2[0], dim)
    g = capi.GMG(H)
    g.set_coefficient(g.new_face_vector(0, random_beta(levels[0].P * pu.face_size(n, dim), 7)))
    betas = device_betas(g, levels, n, dim)
    for l, L in enumerate(levels):
        u, f = util.rand_vec(L.size, 120 + l), util.rand_vec(L.size, 130 + l)
        du, df = g.new_vector(l, u), g.new_vector(l, f)
        g.smooth(df, du, level=l, smoother=capi.SMOOTH_RBGS)
        err = rel(du.download(), vc.rbgs(L, betas[l], f, u))
        print(f"128^2 sweep level {l}: {err:.3e}")
        assert err <= 1e-11, l


def test_restriction_and_coefficient_levels(case):
    g, n, dim, levels = case["g"], case["n"], case["dim"], case["levels"]
    betas = case["betas"]
    assert np.array_equal(pu.pack(*betas[0]), case["beta0"])
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        want = vc.restrict_faces(F, C, betas[l])
        tol = 4 * util.EPS * max(betas[l][0].max(), betas[l][1].max())
        err = max(np.abs(betas[l + 1][0] - want[0]).max(), np.abs(betas[l + 1][1] - want[1]).max())
        print(f"coefficient level {l + 1}: {err:.3e} (bound {tol:.3e})")
        assert err <= tol, l
        dF, dC = g.new_face_vector(l, pu.pack(*betas[l])), g.new_face_vector(l + 1)
        g.faces_restrict(l, dF, dC)
        assert np.array_equal(dC.download(), pu.pack(*betas[l + 1])), l
        for pf in range(F.P):
            if F.a["orth_on_parent"][pf] < 0:
                pc = F.a["parent"][pf]
                assert np.array_equal(betas[l + 1][0][pc], betas[l][0][pf]) and np.array_equal(betas[l + 1][1][pc], betas[l][1][pf]), (l, pf)
    # a second call with other data updates every level; then back, for the tests that follow
    other = random_beta(case["beta0"].size, 8)
    g.set_coefficient(g.new_face_vector(0, other))
    again = device_betas(g, levels, n, dim)
    chain = vc.restrict_all(levels, pu.unpack(other, n, dim))
    for l in range(len(levels)):
        assert not np.array_equal(again[l][0], betas[l][0]), l
        assert np.abs(again[l][0] - chain[l][0]).max() <= 4 * (l + 1) * util.EPS * 2.0 and np.abs(again[l][1] - chain[l][1]).max() <= 4 * (l + 1) * util.EPS * 2.0, l
    g.set_coefficient(g.new_face_vector(0, case["beta0"]))
    back = device_betas(g, levels, n, dim)
    for l in range(len(levels)):
        assert np.array_equal(back[l][0], betas[l][0]) and np.array_equal(back[l][1], betas[l][1]), l


@pytest.mark.parametrize("interp", [capi.INTERP_DIRECT, capi.INTERP_LINEAR], ids=["direct", "linear"])
@pytest.mark.parametrize("cycle_type", [0, 1], ids=["V", "W"])
@pytest.mark.parametrize("sm", [capi.SMOOTH_RBGS, capi.SMOOTH_JACOBI], ids=["rbgs", "jacobi"])
def test_beta_two_is_the_constant_coefficient_cycle(case, sm, cycle_type, interp):
    g, L = case["g"], case["levels"][0]
    f = util.rand_vec(L.size, 140)
    df, dh, du, dv = g.new_vector(0, f), g.new_vector(0, f / 2), g.new_vector(0), g.new_vector(0)
    two = g.new_face_vector(0)
    two.set(2.0)
    g.set_interpolator(interp)
    try:
        g.set_coefficient(two)
        got = {}
        for fuse in (0, 3):
            g.cycle(g.default_opts(smoother=sm, cycle_type=cycle_type, coarse_sweeps=3, fuse=fuse), df, du)
            got[fuse] = du.download()
        assert np.array_equal(got[0], got[3])
        g.set_coefficient(None)
        assert not g.has_coefficient()
        g.cycle(g.default_opts(smoother=sm, cycle_type=cycle_type, coarse_sweeps=3, fuse=0, exact_coarse=0), dh, dv)
        err = rel(got[0], dv.download())
        print(f"beta = 2 against the constant-coefficient cycle: {err:.3e}")
        assert err <= 1e-10
    finally:
        g.set_interpolator(capi.INTERP_DIRECT)
        g.set_coefficient(g.new_face_vector(0, case["beta0"]))


# ---- against the CPU composition: the meshes of tests/test_varcoef_host.py (varcoef_util.SOLVES)
@pytest.mark.parametrize("interp", [capi.INTERP_DIRECT, capi.INTERP_LINEAR], ids=["direct", "linear"])
@pytest.mark.parametrize("beta_fn", [vc.smooth_beta, vc.jump_beta], ids=["smooth", "jump"])
@pytest.mark.parametrize("name,n,div,dim", SOLVES, ids=lambda v: str(v))
def test_cycle_and_solve_against_the_cpu_composition(name, n, div, dim, beta_fn, interp):
    H, levels, g = solve_setup(name, n, div, dim)
    L = levels[0]
    beta0 = vc.beta_from(H.tables(0), n, dim, beta_fn)
    betas = vc.restrict_all(levels, beta0)
    prolong = prolong_util.direct if interp == capi.INTERP_DIRECT else prolong_util.prolong_linear_add
    coarse = 32 if dim == 2 else 16
    b = util.rand_vec(L.size, 5)
    g.set_interpolator(interp)
    try:
        g.set_coefficient(g.new_face_vector(0, pu.pack(*beta0)))
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=coarse)
        db, du = g.new_vector(0, b), g.new_vector(0)
        g.cycle(o, db, du)
        err = rel(du.download(), vc.cycle(levels, betas, b, prolong, coarse=coarse))
        print(f"cycle: {err:.3e}")
        assert err <= 1e-10
        x_ref, its_ref = vc.bicgstab(levels, betas, b, prolong, tol=1e-10, coarse=coarse)
        dx = g.new_vector(0)
        its, rr = g.bicgstab(dx, db, o, tol=1e-10, max_it=40)
        print(f"solve: {its} iterations on the device, {its_ref} in the composition, relative residual {rr:.2e}")
        assert rr <= 1e-10 and abs(its - its_ref) <= 1
        assert rel(dx.download(), x_ref) <= 1e-8
    finally:
        g.set_interpolator(capi.INTERP_DIRECT)
        g.set_coefficient(None)


@pytest.mark.parametrize("name,n,div,dim", [("uniform", 8, 3, 2), ("uniform", 8, 2, 3)], ids=["2d", "3d"])
def test_manufactured_solve_and_projection(name, n, div, dim):
    H, levels, g = solve_setup(name, n, div, dim)
    L = levels[0]
    betas, rhs, exact = vc.manufactured_problem(H, levels, n, dim, *(vc.manufactured2d() if dim == 2 else vc.manufactured3d()))
    coarse = 32 if dim == 2 else 16
    x_ref, _ = vc.bicgstab(levels, betas, rhs, prolong_util.direct, tol=1e-12, coarse=coarse)
    dbeta = g.new_face_vector(0, pu.pack(*betas[0]))
    try:
        g.set_coefficient(dbeta)
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=coarse)
        dx, db = g.new_vector(0), g.new_vector(0, rhs)
        its, rr = g.bicgstab(dx, db, o, tol=1e-12, max_it=60)
        e_dev, e_ref = np.abs(dx.download() - exact).max(), np.abs(x_ref - exact).max()
        print(f"{dim}d: {its} iterations, max error device {e_dev:.6e} composition {e_ref:.6e}")
        assert rr <= 1e-12 and abs(e_dev - e_ref) <= 1e-8 * e_ref
        # the variable-density projection: U = U* - beta (.) grad p with A_b p = div U*
        Ustar = util.rand_vec(L.P * pu.face_size(n, dim), 200)
        dU, df, dp, dr, dd, dG = g.new_face_vector(0, Ustar), g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_face_vector(0)
        g.divergence(dU, df)
        its, rr = g.bicgstab(dp, df, o, tol=1e-12, max_it=60)
        assert rr <= 1e-12
        g.residual(dp, df, dr)
        g.gradient(dp, dG)
        dG.multiply(dbeta)
        dU.addScaled(-1.0, dG)
        g.divergence(dU, dd)
        bmax = max(betas[0][0].max(), betas[0][1].max())
        bound = dr.infNorm() + 2 * bmax * util.op_tol(L, dp.download()) + 4 * util.EPS * 2 * dim / L.a["h"].min() * np.abs(Ustar).max()
        print(f"{dim}d projection: max|div U*| {df.infNorm():.3e} -> max|div U| {dd.infNorm():.3e}, bound {bound:.3e}")
        assert dd.infNorm() <= bound
    finally:
        g.set_coefficient(None)


# ---- state
def test_clearing_the_coefficient_gives_the_old_bits_back():
    m, H, levels = util.setup("2refine.bin", 8, 1)
    g = capi.GMG(H)
    f = g.new_vector(0, util.rand_vec(levels[0].size, 3))
    u = g.new_vector(0)
    g.cycle(g.default_opts(), f, u)
    before = u.checksumLocal()
    g.set_coefficient(g.new_face_vector(0, random_beta(levels[0].P * pu.face_size(8, 3), 9)))
    g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), f, u)
    assert u.checksumLocal() != before
    g.set_coefficient(None)
    g.release_workspace()  # (cleared: the per-level copies go too; the next set_coefficient makes them again)
    g.cycle(g.default_opts(), f, u)
    assert u.checksumLocal() == before
    g.set_coefficient(g.new_face_vector(0, random_beta(levels[0].P * pu.face_size(8, 3), 9)))
    assert g.has_coefficient()


def test_calls_without_a_variable_coefficient_form_are_refused():
    m, H, levels = util.setup("2refine.bin", 8, 0)
    g = capi.GMG(H)
    L = levels[0]
    u, f, r = g.new_vector(0), g.new_vector(0, util.rand_vec(L.size, 1)), g.new_vector(0)
    beta = g.new_face_vector(0)
    beta.set(1.5)
    with pytest.raises(capi.TeError) as e:
        g.coefficient(0, g.new_face_vector(0))
    assert e.value.code == capi.TE_ESTATE
    for bad in (u, g.new_face_vector(1)):
        with pytest.raises(capi.TeError) as e:
            g.set_coefficient(bad)
        assert e.value.code == capi.TE_EINVAL
    with pytest.raises(capi.TeError) as e:
        g.faces_restrict(0, beta, g.new_face_vector(0))
    assert e.value.code == capi.TE_EINVAL
    with pytest.raises(capi.TeError) as e:
        g.faces_restrict(g.num_levels - 1, g.new_face_vector(g.num_levels - 1), g.new_face_vector(g.num_levels - 1))
    assert e.value.code == capi.TE_EINVAL
    g.set_coefficient(beta)
    gam = g.new_iface_vector(0)
    for call in (lambda: g.fmg(f, u, g.default_opts()), lambda: g.patch_apply(u, r), lambda: g.iface_interp(u, gam),
                 lambda: g.apply_with_interface(u, gam, r), lambda: g.add_iface_rhs(gam, r), lambda: g.solve_with_interface(f, u, gam),
                 lambda: g.schur_apply(gam, g.new_iface_vector(0)), lambda: g.schur_cheb(gam, g.new_iface_vector(0)), lambda: g.schur_solve(f, u, gam)):
        refused(call, capi.TE_ESTATE, "coefficient")
    for sm in (capi.SMOOTH_PATCH_SOLVE, capi.SMOOTH_PATCH_BCGS):
        refused(lambda: g.smooth(f, u, smoother=sm), capi.TE_EUNSUPPORTED)
        refused(lambda: g.cycle(g.default_opts(smoother=sm), f, u), capi.TE_EUNSUPPORTED)
    # te_gmg_release_workspace while a coefficient is set keeps the per-level copies: the operator does not change
    A0, A1, chk = g.new_vector(0), g.new_vector(0), g.new_face_vector(g.num_levels - 1)
    g.apply(f, A0)
    g.release_workspace()
    assert g.has_coefficient()
    g.coefficient(g.num_levels - 1, chk)
    assert np.array_equal(chk.download(), np.full(chk.size, 1.5))
    g.apply(f, A1)
    assert np.array_equal(A0.download(), A1.download())
    g.set_coefficient(None)
    g.patch_apply(u, r)  # cleared: available again


def test_sharded_hierarchies_are_refused():
    m = util.mesh("uniform", 2)
    gs = capi.GMG(capi.Hierarchy(m, 4, rank=0, nranks=2))
    for call in (lambda: gs.set_coefficient(gs.new_face_vector(0)), lambda: gs.faces_restrict(0, gs.new_face_vector(0), gs.new_face_vector(1))):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_ESTATE and "sharded" in str(e.value)


def test_vec_multiply():
    m, H, levels = util.setup("2refine.bin", 4, 0)
    g = capi.GMG(H)
    makers = (g.new_vector, g.new_iface_vector, g.new_boundary_vector, g.new_face_vector)
    for k, make in enumerate(makers):
        for l in range(g.num_levels):
            size = make(l).size
            if size == 0:
                continue
            a, b = util.rand_vec(size, 10 + k), util.rand_vec(size, 20 + k)
            da, db = make(l, a), make(l, b)
            da.multiply(db)
            assert np.array_equal(da.download(), a * b), (k, l)
            assert np.array_equal(db.download(), b)
    with pytest.raises(capi.TeError) as e:
        g.new_vector(0).multiply(g.new_face_vector(0))
    assert e.value.code == capi.TE_EINVAL
    with pytest.raises(capi.TeError) as e:
        g.new_vector(0).multiply(g.new_vector(1))
    assert e.value.code == capi.TE_EINVAL


def test_profile_rows_show_the_new_classes_only():
    m, H, levels = util.setup("uniform", 8, 2)
    g = capi.GMG(H)
    beta = g.new_face_vector(0)
    beta.set(1.25)
    f, u = g.new_vector(0, util.rand_vec(levels[0].size, 3)), g.new_vector(0)
    g.profile(True)
    g.profile_reset()
    g.set_coefficient(beta)
    g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), f, u)
    g.cycle(g.default_opts(smoother=capi.SMOOTH_JACOBI), f, u)
    g.apply(u, g.new_vector(0))
    rows = g.profile_rows()
    g.profile(False)
    for k in ("apply_coef", "resid_coef", "jacobi_coef", "rbgs_coef", "faces_restrict"):
        assert rows[k]["calls"] > 0 and rows[k]["cells"] > 0, (k, sorted(rows))
    assert not [k for k in rows if k.startswith("stencil_") or k.startswith("rbgs_") and k != "rbgs_coef" or k.startswith("patch_solve")], sorted(rows)
