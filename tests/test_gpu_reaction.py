"""-m gpu: the reaction term A_bs u = div(beta grad u) - sigma u (include/te_hip.h te_gmg_set_reaction and what follows it) against the
numpy statement of tests/varcoef_util.py with sigma (tests/reaction_util.py holds what is sigma's own), which tests/test_reaction_host.py
pins to the statement without sigma and the oracle.

Bounds (none of them comes from what the kernels give):
  apply / residual   max(beta) * util.op_tol(u) + 4 eps max(sigma) max|u|: section 18's bound plus one multiplication and one subtraction
  residual norm      1e-13 relative against numpy's sum over the downloaded residual (another summation order)
  one sweep          1e-11 relative 2-norm, the project's sweep figure (test_gpu_parity.py)
  slab matrix        bit for bit against the TE_ZS_PIN = 1 result, and the two bounds above against the numpy statement
  sigma levels       4 eps max(sigma) (te_restrict's average: additions and a multiplication by a power of two); copy-through bit for bit
  sigma = 0          1e-10 relative against the beta-only result (only d + 0 and - 0 * u enter); clearing gives the old BITS back
  cycle / solve      1e-10 relative; iteration count +-1 and 1e-8 relative: the conventions of test_gpu_parity.py
  manufactured       solve to 1e-12 within 1e-8 relative of the CPU composition's, error against the exact u within 1 % of its error"""
import contextlib

import numpy as np
import pytest

from pressurepoissonsolver_amd import capi
from tests import bc_util, projection_util as pu, prolong_util, reaction_util as ru, util, varcoef_util as vc
from tests.reaction_util import device_sigmas, random_sigma
from tests.varcoef_util import CASES, SOLVES, device_betas, random_beta, refused, rel, solve_setup

pytestmark = pytest.mark.gpu

OMEGA = 6.0 / 7.0


def op_bound(L, beta, sigma, u):
    return max(beta[0].max(), beta[1].max()) * util.op_tol(L, u) + 4 * util.EPS * sigma.max() * np.abs(u).max()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-d{c[1]}-n{c[2]}-{c[3]}d-{c[4]:06b}")
def case(request):
    name, div, n, dim, mask = request.param
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    g = capi.GMG(H)
    beta0, sigma0 = random_beta(levels[0].P * pu.face_size(n, dim), 7), random_sigma(levels[0].size, 17)
    g.set_coefficient(g.new_face_vector(0, beta0))
    assert not g.has_reaction()
    g.set_reaction(g.new_vector(0, sigma0))  # (the caller's vector goes away: the solver has its copy)
    assert g.has_reaction() and g.has_coefficient()
    return dict(H=H, levels=levels, g=g, n=n, dim=dim, mask=mask, beta0=beta0, sigma0=sigma0, betas=device_betas(g, levels, n, dim),
                sigmas=device_sigmas(g, levels))


def test_apply_and_residual(case):
    g = case["g"]
    for l, L in enumerate(case["levels"]):
        beta, sigma = case["betas"][l], case["sigmas"][l]
        u, f = util.rand_vec(L.size, 100 + l), util.rand_vec(L.size, 110 + l)
        du, df, dA, dr = g.new_vector(l, u), g.new_vector(l, f), g.new_vector(l), g.new_vector(l)
        g.apply(du, dA, level=l)
        A, want = dA.download(), vc.apply(L, beta, u, sigma)
        tol = op_bound(L, beta, sigma, u)
        err = np.abs(A - want).max()
        print(f"apply level {l}: {err / tol:.3f} of the bound")
        assert err <= tol, l
        assert np.abs(want - vc.apply(L, beta, u)).max() > 100 * tol  # (sigma is seen at all)
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
    for l, L in enumerate(case["levels"]):
        beta, sigma = case["betas"][l], case["sigmas"][l]
        u, f = util.rand_vec(L.size, 120 + l), util.rand_vec(L.size, 130 + l)
        for sm, want in ((capi.SMOOTH_RBGS, vc.rbgs(L, beta, f, u, sigma)), (capi.SMOOTH_JACOBI, vc.jacobi(L, beta, f, u, OMEGA, sigma))):
            du, df = g.new_vector(l, u), g.new_vector(l, f)
            g.smooth(df, du, level=l, smoother=sm, omega=OMEGA)
            err = rel(du.download(), want)
            print(f"sweep {sm} level {l}: {err:.3e}")
            assert err <= 1e-11, (l, sm)


def test_sweep_above_the_lds_limit():
    """2D patches of 128^2 do not fit the LDS form (n <= 64): the two colour launches k_coef_rbgs2d<0 / 1, SIG>"""
    n, dim = 128, 2
    m, H, levels = bc_util.setup("2d2ref.bin", n, 0, bc_util.MASKS2[0], dim)
    g = capi.GMG(H)
    g.set_coefficient(g.new_face_vector(0, random_beta(levels[0].P * pu.face_size(n, dim), 7)))
    g.set_reaction(g.new_vector(0, random_sigma(levels[0].size, 17)))
    betas, sigmas = device_betas(g, levels, n, dim), device_sigmas(g, levels)
    for l, L in enumerate(levels):
        u, f = util.rand_vec(L.size, 120 + l), util.rand_vec(L.size, 130 + l)
        du, df = g.new_vector(l, u), g.new_vector(l, f)
        g.smooth(df, du, level=l, smoother=capi.SMOOTH_RBGS)
        err = rel(du.download(), vc.rbgs(L, betas[l], f, u, sigmas[l]))
        print(f"128^2 sweep level {l}: {err:.3e}")
        assert err <= 1e-11, l


def test_reaction_levels(case):
    g, levels, sigmas = case["g"], case["levels"], case["sigmas"]
    assert np.array_equal(sigmas[0], case["sigma0"])
    want = ru.restrict_all(levels, case["sigma0"])
    tol = 4 * util.EPS * case["sigma0"].max()
    for l in range(1, len(levels)):
        err = np.abs(sigmas[l] - want[l]).max()
        print(f"sigma level {l}: {err:.3e} (bound {tol:.3e})")
        assert err <= tol, l
        F = levels[l - 1]
        fine, coarse = sigmas[l - 1].reshape(F.P, -1), sigmas[l].reshape(levels[l].P, -1)
        for pf in range(F.P):
            if F.a["orth_on_parent"][pf] < 0:
                assert np.array_equal(coarse[F.a["parent"][pf]], fine[pf]), (l, pf)
    # a second call with other data updates every level (the buffers are reused); then back, for the tests that follow
    other = random_sigma(case["sigma0"].size, 18)
    g.set_reaction(g.new_vector(0, other))
    again, chain = device_sigmas(g, levels), ru.restrict_all(levels, other)
    for l in range(len(levels)):
        assert not np.array_equal(again[l], sigmas[l]) and np.abs(again[l] - chain[l]).max() <= 4 * util.EPS * other.max(), l
    g.set_reaction(g.new_vector(0, case["sigma0"]))
    for l, back in enumerate(device_sigmas(g, levels)):
        assert np.array_equal(back, sigmas[l]), l


# ---- every admitted (patch size, z-slab count) pair: the slab seams are where a sigma ring can be one plane off
PIN = "TE_ZS_PIN"
COUNTS = {8: (1, 2), 16: (1, 2, 4), 32: (1, 2, 4, 8)}


@contextlib.contextmanager
def pinned(g, zs):
    try:
        g.set_option(PIN, zs)
        yield
    finally:
        g.set_option(PIN, None)


@pytest.mark.parametrize("n", sorted(COUNTS))
def test_slab_matrix(n):
    m, H, levels = bc_util.setup("uniform", n, 1, bc_util.CHANNEL)
    g = capi.GMG(H)
    g.set_coefficient(g.new_face_vector(0, random_beta(levels[0].P * pu.face_size(n, 3), 7)))
    g.set_reaction(g.new_vector(0, random_sigma(levels[0].size, 17)))
    betas, sigmas = device_betas(g, levels, n, 3), device_sigmas(g, levels)
    inputs = [(util.rand_vec(L.size, 100 + l), util.rand_vec(L.size, 110 + l)) for l, L in enumerate(levels)]
    refs = [(vc.apply(L, betas[l], u, sigmas[l]), vc.rbgs(L, betas[l], f, u, sigmas[l]), vc.jacobi(L, betas[l], f, u, OMEGA, sigmas[l]))
            for l, (L, (u, f)) in enumerate(zip(levels, inputs))]
    base = None
    for zs in COUNTS[n]:
        got = []
        with pinned(g, zs):
            for l, L in enumerate(levels):
                assert g.slab_count(l, capi.SLABS_STENCIL) == zs and g.slab_count(l, capi.SLABS_SWEEP) == zs, (n, zs, l)
                u, f = inputs[l]
                du, df, dA, dr = g.new_vector(l, u), g.new_vector(l, f), g.new_vector(l), g.new_vector(l)
                g.apply(du, dA, level=l)
                g.residual(du, df, dr, level=l)
                ds, dj = g.new_vector(l, u), g.new_vector(l, u)
                g.smooth(df, ds, level=l, smoother=capi.SMOOTH_RBGS)
                g.smooth(df, dj, level=l, smoother=capi.SMOOTH_JACOBI, omega=OMEGA)
                got.append((dA.download(), ds.download(), dr.download(), dj.download()))
        if base is None:
            base = got
        for l, L in enumerate(levels):
            u, f = inputs[l]
            for k in range(4):
                assert np.array_equal(got[l][k], base[l][k]), (n, zs, l, k)
            tol = op_bound(L, betas[l], sigmas[l], u)
            assert np.abs(got[l][0] - refs[l][0]).max() <= tol, (n, zs, l)
            assert np.abs(got[l][2] - (f - refs[l][0])).max() <= tol, (n, zs, l)
            assert rel(got[l][1], refs[l][1]) <= 1e-11, (n, zs, l)
            assert rel(got[l][3], refs[l][2]) <= 1e-11, (n, zs, l)


# ---- sigma = 0 on the device, and the lifetime rule
@pytest.mark.parametrize("name,n,div,dim", [("2refine.bin", 8, 1, 3), ("2d2ref.bin", 8, 2, 2)], ids=["3d", "2d"])
def test_sigma_zero_and_clearing(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    g = capi.GMG(H)
    L = levels[0]
    f = g.new_vector(0, util.rand_vec(L.size, 3))
    u, x = g.new_vector(0), g.new_vector(0)
    o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=16)
    g.cycle(g.default_opts(), f, u)
    constant = u.download()
    beta = g.new_face_vector(0, random_beta(L.P * pu.face_size(n, dim), 9))

    def beta_only_run():
        g.cycle(o, f, u)
        x.set(0.0)
        its, _ = g.bicgstab(x, f, o, tol=1e-10, max_it=40)
        return u.download(), x.download(), its

    g.set_coefficient(beta)
    cyc_b, sol_b, its_b = beta_only_run()
    zero = g.new_vector(0)
    g.set_reaction(zero)
    assert g.has_reaction()
    g.cycle(o, f, u)
    x.set(0.0)
    its, _ = g.bicgstab(x, f, o, tol=1e-10, max_it=40)
    print(f"sigma = 0: cycle {rel(u.download(), cyc_b):.3e}, solve {rel(x.download(), sol_b):.3e}, {its} / {its_b} iterations")
    assert rel(u.download(), cyc_b) <= 1e-10 and rel(x.download(), sol_b) <= 1e-10 and its == its_b
    # a sigma run, then NULL: the beta-only bits
    g.set_reaction(g.new_vector(0, random_sigma(L.size, 17)))
    g.cycle(o, f, u)
    assert not np.array_equal(u.download(), cyc_b)
    g.set_reaction(None)
    assert not g.has_reaction() and g.has_coefficient()
    with pytest.raises(capi.TeError) as e:
        g.reaction(0, g.new_vector(0))
    assert e.value.code == capi.TE_ESTATE
    g.release_workspace()  # (sigma cleared, the coefficient set: the sigma buffers go, the operator stays)
    got = beta_only_run()
    assert np.array_equal(got[0], cyc_b) and np.array_equal(got[1], sol_b) and got[2] == its_b
    # a sigma run, then te_gmg_set_coefficient: sigma is cleared with it
    g.set_reaction(g.new_vector(0, random_sigma(L.size, 17)))
    g.release_workspace()  # (set: stays)
    assert g.has_reaction()
    g.cycle(o, f, u)
    assert not np.array_equal(u.download(), cyc_b)
    g.set_coefficient(beta)
    assert not g.has_reaction()
    got = beta_only_run()
    assert np.array_equal(got[0], cyc_b) and np.array_equal(got[1], sol_b) and got[2] == its_b
    # a sigma run, then no coefficient at all: the constant-coefficient bits
    g.set_reaction(g.new_vector(0, random_sigma(L.size, 17)))
    g.cycle(o, f, u)
    g.set_coefficient(None)
    assert not g.has_reaction() and not g.has_coefficient()
    g.release_workspace()
    g.cycle(g.default_opts(), f, u)
    assert np.array_equal(u.download(), constant)


# ---- against the CPU composition: the meshes of tests/test_reaction_host.py (varcoef_util.SOLVES)
@pytest.mark.parametrize("interp", [capi.INTERP_DIRECT, capi.INTERP_LINEAR], ids=["direct", "linear"])
@pytest.mark.parametrize("beta_fn", [vc.smooth_beta, vc.jump_beta], ids=["smooth", "jump"])
@pytest.mark.parametrize("name,n,div,dim", SOLVES, ids=lambda v: str(v))
def test_cycle_and_solve_against_the_cpu_composition(name, n, div, dim, beta_fn, interp):
    H, levels, g = solve_setup(name, n, div, dim)
    L = levels[0]
    beta0 = vc.beta_from(H.tables(0), n, dim, beta_fn)
    betas = vc.restrict_all(levels, beta0)
    sigmas = ru.restrict_all(levels, random_sigma(L.size, 17))
    prolong = prolong_util.direct if interp == capi.INTERP_DIRECT else prolong_util.prolong_linear_add
    coarse = 32 if dim == 2 else 16
    b = util.rand_vec(L.size, 5)
    g.set_interpolator(interp)
    try:
        g.set_coefficient(g.new_face_vector(0, pu.pack(*beta0)))
        g.set_reaction(g.new_vector(0, sigmas[0]))
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=coarse)
        db, du = g.new_vector(0, b), g.new_vector(0)
        g.cycle(o, db, du)
        err = rel(du.download(), vc.cycle(levels, betas, b, prolong, sigmas=sigmas, coarse=coarse))
        print(f"cycle: {err:.3e}")
        assert err <= 1e-10
        x_ref, its_ref = vc.bicgstab(levels, betas, b, prolong, tol=1e-10, sigmas=sigmas, coarse=coarse)
        dx = g.new_vector(0)
        its, rr = g.bicgstab(dx, db, o, tol=1e-10, max_it=40)
        print(f"solve: {its} iterations on the device, {its_ref} in the composition, relative residual {rr:.2e}")
        assert rr <= 1e-10 and abs(its - its_ref) <= 1
        assert rel(dx.download(), x_ref) <= 1e-8
    finally:
        g.set_interpolator(capi.INTERP_DIRECT)
        g.set_coefficient(None)


@pytest.mark.parametrize("cycle_type", [0, 1], ids=["V", "W"])
def test_jacobi_and_w_cycles_against_the_cpu_composition(cycle_type):
    name, n, div, dim = SOLVES[3]
    H, levels, g = solve_setup(name, n, div, dim)
    beta0 = vc.beta_from(H.tables(0), n, dim, vc.smooth_beta)
    betas, sigmas = vc.restrict_all(levels, beta0), ru.restrict_all(levels, random_sigma(levels[0].size, 17))
    b = util.rand_vec(levels[0].size, 5)
    try:
        g.set_coefficient(g.new_face_vector(0, pu.pack(*beta0)))
        g.set_reaction(g.new_vector(0, sigmas[0]))
        db, du = g.new_vector(0, b), g.new_vector(0)
        for sm in (capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS):
            g.cycle(g.default_opts(smoother=sm, cycle_type=cycle_type, coarse_sweeps=4), db, du)
            err = rel(du.download(), vc.cycle(levels, betas, b, prolong_util.direct, sigmas=sigmas, smoother=sm, cycle_type=cycle_type, coarse=4))
            print(f"cycle type {cycle_type} smoother {sm}: {err:.3e}")
            assert err <= 1e-10
    finally:
        g.set_coefficient(None)


@pytest.mark.parametrize("name,n,div,dim", [("uniform", 8, 3, 2), ("uniform", 8, 2, 3)], ids=["2d", "3d"])
def test_manufactured_implicit_diffusion_step(name, n, div, dim):
    H, levels, g = solve_setup(name, n, div, dim)
    betas, sigmas, rhs, exact = ru.manufactured_problem(H, levels, n, dim, *(ru.manufactured2d() if dim == 2 else ru.manufactured3d()))
    coarse = 32 if dim == 2 else 16
    x_ref, _ = vc.bicgstab(levels, betas, rhs, prolong_util.direct, tol=1e-12, sigmas=sigmas, coarse=coarse)
    try:
        g.set_coefficient(g.new_face_vector(0, pu.pack(*betas[0])))
        g.set_reaction(g.new_vector(0, sigmas[0]))
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=coarse)
        dx, db = g.new_vector(0), g.new_vector(0, rhs)
        its, rr = g.bicgstab(dx, db, o, tol=1e-12, max_it=60)
        x = dx.download()
        e_dev, e_ref = np.abs(x - exact).max(), np.abs(x_ref - exact).max()
        print(f"{dim}d: {its} iterations, max error device {e_dev:.6e} composition {e_ref:.6e}, x against the composition {rel(x, x_ref):.3e}")
        assert rr <= 1e-12 and rel(x, x_ref) <= 1e-8
        assert abs(e_dev - e_ref) <= 0.01 * e_ref
    finally:
        g.set_coefficient(None)


# ---- state
def test_refusals_and_argument_checks():
    m, H, levels = util.setup("2refine.bin", 8, 0)
    g, other = capi.GMG(H), capi.GMG(H)
    L = levels[0]
    u, f, r = g.new_vector(0), g.new_vector(0, util.rand_vec(L.size, 1)), g.new_vector(0)
    sigma = g.new_vector(0)
    sigma.set(3.0)
    assert not g.has_reaction()
    with pytest.raises(capi.TeError) as e:  # sigma lives on the coefficient path only
        g.set_reaction(sigma)
    assert e.value.code == capi.TE_ESTATE and "coefficient" in str(e.value)
    g.set_reaction(None)  # (nothing to clear)
    with pytest.raises(capi.TeError) as e:
        g.reaction(0, g.new_vector(0))
    assert e.value.code == capi.TE_ESTATE
    beta = g.new_face_vector(0)
    beta.set(1.0)
    g.set_coefficient(beta)
    for bad in (g.new_face_vector(0), g.new_iface_vector(0), g.new_boundary_vector(0), g.new_vector(1), other.new_vector(0)):
        with pytest.raises(capi.TeError) as e:
            g.set_reaction(bad)
        assert e.value.code == capi.TE_EINVAL
        assert not g.has_reaction()
    g.set_reaction(sigma)
    assert g.has_reaction()
    for bad in (g.new_face_vector(0), g.new_vector(1)):
        with pytest.raises(capi.TeError) as e:
            g.reaction(0, bad)
        assert e.value.code == capi.TE_EINVAL
    with pytest.raises(capi.TeError) as e:  # a failed call leaves no sigma set
        g.set_reaction(g.new_face_vector(0))
    assert e.value.code == capi.TE_EINVAL
    g.set_reaction(sigma)
    gam = g.new_iface_vector(0)
    for call in (lambda: g.fmg(f, u, g.default_opts()), lambda: g.patch_apply(u, r), lambda: g.iface_interp(u, gam),
                 lambda: g.apply_with_interface(u, gam, r), lambda: g.add_iface_rhs(gam, r), lambda: g.solve_with_interface(f, u, gam),
                 lambda: g.schur_apply(gam, g.new_iface_vector(0)), lambda: g.schur_cheb(gam, g.new_iface_vector(0)), lambda: g.schur_solve(f, u, gam)):
        refused(call, capi.TE_ESTATE, "coefficient")
    for sm in (capi.SMOOTH_PATCH_SOLVE, capi.SMOOTH_PATCH_BCGS):
        refused(lambda: g.smooth(f, u, smoother=sm), capi.TE_EUNSUPPORTED)
        refused(lambda: g.cycle(g.default_opts(smoother=sm), f, u), capi.TE_EUNSUPPORTED)
    # beta = 1 and a constant sigma: Laplace(u) - sigma u, the recipe of the header
    A, lap = g.new_vector(0), g.new_vector(0)
    g.apply(f, A)
    g.set_coefficient(None)
    g.apply(f, lap)
    want = lap.download() - 3.0 * f.download()
    assert np.abs(A.download() - want).max() <= util.op_tol(L, f.download()) + 4 * util.EPS * 3.0
    g.patch_apply(u, r)  # cleared: available again


def test_sharded_hierarchies_are_refused():
    m = util.mesh("uniform", 2)
    gs = capi.GMG(capi.Hierarchy(m, 4, rank=0, nranks=2))
    with pytest.raises(capi.TeError) as e:
        gs.set_reaction(gs.new_vector(0))
    assert e.value.code == capi.TE_ESTATE and "sharded" in str(e.value)
    assert not gs.has_reaction()


def test_profile_rows_without_sigma_are_what_they_were():
    m, H, levels = util.setup("uniform", 8, 2)
    g = capi.GMG(H)
    beta = g.new_face_vector(0)
    beta.set(1.25)
    f, u = g.new_vector(0, util.rand_vec(levels[0].size, 3)), g.new_vector(0)

    def rows_of(sigma):
        g.profile(True)
        g.profile_reset()
        g.set_coefficient(beta)
        if sigma is not None:
            g.set_reaction(sigma)
        g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), f, u)
        g.cycle(g.default_opts(smoother=capi.SMOOTH_JACOBI), f, u)
        g.apply(u, g.new_vector(0))
        rows = g.profile_rows()
        g.profile(False)
        g.set_coefficient(None)
        return {k: (v["calls"], v["cells"]) for k, v in rows.items() if v["calls"] > 0}

    without = rows_of(None)
    for k in ("apply_coef", "resid_coef", "jacobi_coef", "rbgs_coef", "faces_restrict"):
        assert k in without, sorted(without)
    assert not [k for k in without if k.startswith("stencil_") or k.startswith("rbgs_") and k != "rbgs_coef" or k.startswith("patch_solve")], sorted(without)
    sig = g.new_vector(0)
    sig.set(2.0)
    with_sigma = rows_of(sig)
    # the sigma run uses the same classes with the same calls and cells; te_gmg_set_reaction's restriction adds to te_restrict's row
    for k in ("apply_coef", "resid_coef", "jacobi_coef", "rbgs_coef", "faces_restrict"):
        assert with_sigma[k] == without[k], k
    assert set(with_sigma) == set(without)
    assert rows_of(None) == without
