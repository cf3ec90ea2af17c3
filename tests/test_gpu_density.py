"""-m gpu: te_faces_from_cells, te_project_weighted and te_add_boundary_rhs_weighted (include/te_hip.h) against
the numpy statement of tests/density_util.py, which tests/test_density_host.py checks on its own.

3D runs every admitted (patch size, z-slab count) instantiation of k_cellface3d / k_wproject3d: TE_ZS_PIN chooses the count and
te_gmg_slab_count proves it before every comparison (tests/test_gpu_slab_matrix.py's method), on 8 patches (`uniform`, one divide)
and on 2refine.bin (coarse/fine faces), every level of each, under the channel mask and all-Dirichlet. The statement of a
(mesh, mask, n) is computed once and shared by its slab counts.

Bounds (none of them comes from what the kernels give):
  faces_from_cells   MEAN bit for bit (one addition, one multiplication by a power of two); the division modes 2 eps relative (both
                     sides divide correctly rounded: the bound leaves room for one differing rounding in numerator or quotient)
  project_weighted   |alpha| max(w) grad_tol(p, bd) + 4 eps (max|U| + |alpha| max(w) max|G|): te_project's bound with one more rounding
                     for the product; w = 1: te_project's bits
  weighted fold      4 eps (|f_c| + sum |terms|) per cell; w = 1: te_add_boundary_rhs's bits
  slab counts        every ZS > 1 output equals the ZS = 1 output bit for bit
  whole step         max error against the CPU composition on the statement's beta: 1e-8 relative; max|div U| <= max|f - A_b p|
                     + 2 max(beta) op_tol(p) + 4 eps (2 dim / h_min) max|U*| (test_gpu_varcoef.py's rules)"""
import contextlib
import functools
import types

import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi
from tests import bc_util, density_util as du, projection_util as pu, prolong_util, util, varcoef_util as vc

pytestmark = pytest.mark.gpu

EPS = util.EPS
PIN = "TE_ZS_PIN"
COUNTS = {4: (1,), 8: (1, 2), 16: (1, 2, 4), 32: (1, 2, 4, 8)}  # the admitted pairs: a slab is at least four planes thick
PAIRS = [(n, zs) for n in COUNTS for zs in COUNTS[n]]
CONFIGS3 = [("uniform", 1, bc_util.CHANNEL), ("2refine.bin", 0, bc_util.CHANNEL), ("uniform", 1, 0), ("2refine.bin", 0, 0)]
CASES3 = [c + p for c in CONFIGS3 for p in PAIRS]
IDS3 = [f"{c[0]}-{c[2]:06b}-n{c[3]}-zs{c[4]}" for c in CASES3]
CASES2 = [("2d2ref.bin", 0, bc_util.MASKS2[0], 8), ("2d2ref.bin", 0, 0, 8), ("uniform", 2, bc_util.MASKS2[0], 4), ("uniform", 2, 0, 4)]
IDS2 = [f"{c[0]}-{c[2]:04b}-n{c[3]}" for c in CASES2]
ALPHA = 0.37


def positive(size, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, size)


@functools.lru_cache(maxsize=None)
def solver(name, div, mask, n, dim):
    """one hierarchy and one solver per (mesh, mask, patch size)"""
    orc.set_threads(16)
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    return types.SimpleNamespace(H=H, levels=levels, g=capi.GMG(H), n=n, dim=dim, key=(name, div, mask, n, dim))


@contextlib.contextmanager
def pinned(g, zs):
    try:
        if zs:
            g.set_option(PIN, zs)
        yield
    finally:
        if zs:
            g.set_option(PIN, None)


def reached(g, zs):
    """the rule returns `zs` on every level about to be used -- asked of the solver, not assumed"""
    if zs:
        for l in range(g.num_levels):
            assert g.slab_count(l, capi.SLABS_STENCIL) == zs, (l, zs, g.slab_count(l, capi.SLABS_STENCIL))


# ---- inputs and statements, one per (solver, level): computed once, never changed
@functools.lru_cache(maxsize=None)
def inputs(key, l):
    S = solver(*key)
    L, n, dim = S.levels[l], S.n, S.dim
    fs = L.P * pu.face_size(n, dim)
    nb = pu.num_bfaces(L) * L.nf
    d = types.SimpleNamespace(c=positive(L.size, 300 + l), cb=positive(nb, 310 + l), p=util.rand_vec(L.size, 320 + l), bd=util.rand_vec(nb, 330 + l),
                              U=util.rand_vec(fs, 340 + l), w=positive(fs, 350 + l), f=util.rand_vec(L.size, 360 + l))
    # w and U single-valued on the same-level faces
    pairs = du.same_level_pairs(L)
    for name in ("U", "w"):
        lo, hi = pu.unpack(getattr(d, name), n, dim)
        for p, a, q in pairs:
            sl = [slice(None)] * dim
            sl[dim - 1 - a] = 0
            lo[q, a][tuple(sl)] = hi[p, a]
        setattr(d, name, pu.pack(lo, hi))
    for v in vars(d).values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def faces_statement(key, l, mode, with_cb):
    S, d = solver(*key), inputs(key, l)
    return pu.pack(*du.faces_from_cells(S.levels[l], d.c, mode, d.cb if with_cb else None))


@functools.lru_cache(maxsize=None)
def project_statement(key, l, with_bd):
    S, d = solver(*key), inputs(key, l)
    n, dim = S.n, S.dim
    (lo, hi), G = du.project_weighted(S.levels[l], pu.unpack(d.U, n, dim), d.p, pu.unpack(d.w, n, dim), ALPHA, d.bd if with_bd else None)
    return pu.pack(lo, hi), max(np.abs(G[0]).max(), np.abs(G[1]).max())


# ---- device runs, one per (solver, slab count)
@functools.lru_cache(maxsize=None)
def faces_run(key, zs):
    S = solver(*key)
    g, out = S.g, {}
    with pinned(g, zs):
        reached(g, zs)
        for l, L in enumerate(S.levels):
            d = inputs(key, l)
            dc, dcb, dF = g.new_vector(l, d.c), g.new_boundary_vector(l, d.cb if d.cb.size else None), g.new_face_vector(l)
            for mode in du.MODES:
                for with_cb in (False, True):
                    dF.set(-7.0)
                    g.faces_from_cells(dc, dF, mode=mode, cb=dcb if with_cb else None, level=l)
                    out[l, mode, with_cb] = dF.download()
    return out


@functools.lru_cache(maxsize=None)
def project_run(key, zs):
    S = solver(*key)
    g, out = S.g, {}
    with pinned(g, zs):
        reached(g, zs)
        for l, L in enumerate(S.levels):
            d = inputs(key, l)
            dp, dbd, dw = g.new_vector(l, d.p), g.new_boundary_vector(l, d.bd if d.bd.size else None), g.new_face_vector(l, d.w)
            done = g.new_face_vector(l, np.ones(d.w.size))
            for with_bd in (False, True):
                b = dbd if with_bd else None
                dU = g.new_face_vector(l, d.U)
                g.project_weighted(dU, dp, dw, alpha=ALPHA, bdata=b, level=l)
                out[l, "w", with_bd] = dU.download()
                dU.upload(d.U)
                g.project_weighted(dU, dp, done, alpha=ALPHA, bdata=b, level=l)
                out[l, "one", with_bd] = dU.download()
                dU.upload(d.U)
                g.project(dU, dp, alpha=ALPHA, bdata=b, level=l)
                out[l, "project", with_bd] = dU.download()
    return out


def check_faces(S, got, base=None):
    n, dim = S.n, S.dim
    for l, L in enumerate(S.levels):
        pairs = du.same_level_pairs(L)
        for mode in du.MODES:
            for with_cb in (False, True):
                a, want = got[l, mode, with_cb], faces_statement(S.key, l, mode, with_cb)
                if mode == du.MEAN:
                    assert np.array_equal(a, want), (l, mode, with_cb, np.abs(a - want).max())
                else:
                    rel = np.abs(a - want) / np.abs(want)
                    print(f"level {l} mode {mode} cb={with_cb}: bit-identical {np.array_equal(a, want)}, worst {rel.max() / EPS:.2f} eps")
                    assert (rel <= 2 * EPS).all(), (l, mode, with_cb, rel.max())
                lo, hi = pu.unpack(a, n, dim)
                for p, ax, q in pairs:
                    assert np.array_equal(hi[p, ax], du.lower_face(lo, q, ax, dim)), (l, mode, p, ax)
                if base is not None:
                    assert np.array_equal(a, base[l, mode, with_cb]), (l, mode, with_cb)


def check_project(S, got, base=None):
    n, dim = S.n, S.dim
    for l, L in enumerate(S.levels):
        d = inputs(S.key, l)
        pairs = du.same_level_pairs(L)
        for with_bd in (False, True):
            assert np.array_equal(got[l, "one", with_bd], got[l, "project", with_bd]), (l, with_bd)
            want, gmax = project_statement(S.key, l, with_bd)
            wmax = d.w.max()
            tol = ALPHA * wmax * pu.grad_tol(L, d.p, d.bd if with_bd else None) + 4 * EPS * (np.abs(d.U).max() + ALPHA * wmax * gmax)
            err = np.abs(got[l, "w", with_bd] - want).max()
            print(f"level {l} bdata={with_bd}: {err / tol:.3f} of the bound")
            assert err <= tol, (l, with_bd, err, tol)
            lo, hi = pu.unpack(got[l, "w", with_bd], n, dim)
            for p, ax, q in pairs:
                assert np.array_equal(hi[p, ax], du.lower_face(lo, q, ax, dim)), (l, p, ax)
            if base is not None:
                for k in ("w", "one"):
                    assert np.array_equal(got[l, k, with_bd], base[l, k, with_bd]), (l, k, with_bd)


@pytest.mark.parametrize("name,div,mask,n,zs", CASES3, ids=IDS3)
def test_faces_from_cells_3d(name, div, mask, n, zs):
    S = solver(name, div, mask, n, 3)
    assert len(S.levels) >= 2  # a coarser level as well as level 0
    check_faces(S, faces_run(S.key, zs), faces_run(S.key, 1) if zs > 1 else None)


@pytest.mark.parametrize("name,div,mask,n,zs", CASES3, ids=IDS3)
def test_project_weighted_3d(name, div, mask, n, zs):
    S = solver(name, div, mask, n, 3)
    check_project(S, project_run(S.key, zs), project_run(S.key, 1) if zs > 1 else None)


@pytest.mark.parametrize("name,div,mask,n", CASES2, ids=IDS2)
def test_faces_from_cells_and_project_weighted_2d(name, div, mask, n):
    S = solver(name, div, mask, n, 2)
    assert len(S.levels) >= 2
    check_faces(S, faces_run(S.key, 0))
    check_project(S, project_run(S.key, 0))


FOLDS = [("uniform", 1, bc_util.CHANNEL, 8, 3), ("2refine.bin", 0, bc_util.CHANNEL, 4, 3), ("uniform", 1, 0, 32, 3), ("2d2ref.bin", 0, bc_util.MASKS2[0], 8, 2),
         ("uniform", 2, 0, 4, 2)]


@pytest.mark.parametrize("key", FOLDS, ids=lambda k: f"{k[0]}-{k[2]:06b}-n{k[3]}-{k[4]}d")
def test_weighted_fold(key):
    S = solver(*key)
    g, n, dim = S.g, S.n, S.dim
    for l, L in enumerate(S.levels):
        d = inputs(S.key, l)
        dbd, dw, done = g.new_boundary_vector(l, d.bd), g.new_face_vector(l, d.w), g.new_face_vector(l, np.ones(d.w.size))
        df, d1, d0 = g.new_vector(l, d.f), g.new_vector(l, d.f), g.new_vector(l, d.f)
        g.add_boundary_rhs_weighted(dbd, dw, df, level=l)
        g.add_boundary_rhs_weighted(dbd, done, d1, level=l)
        g.add_boundary_rhs(dbd, d0, level=l)
        assert np.array_equal(d1.download(), d0.download()), l
        want, mag = du.boundary_rhs_weighted(L, pu.unpack(d.w, n, dim), d.bd, d.f)
        err = np.abs(df.download() - want)
        print(f"level {l}: bit-identical {np.array_equal(df.download(), want)}, worst {np.max(err / (4 * EPS * np.maximum(mag, 1e-300))):.3f} of the bound")
        assert (err <= 4 * EPS * mag).all(), l
        assert not np.array_equal(want, d.f)


# ---- the whole step: rho as a cell vector -> beta -> solve -> divergence-free face velocity
@pytest.mark.parametrize("name,n,div,dim", [("uniform", 8, 3, 2), ("uniform", 8, 2, 3), ("2refine.bin", 8, 0, 3)], ids=["2d", "3d", "3d-refined"])
def test_the_whole_step_stays_on_the_device(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    g, L, t = capi.GMG(H), levels[0], H.tables(0)
    beta_fn, u_fn, F_fn = vc.manufactured2d() if dim == 2 else vc.manufactured3d()
    at = lambda fn, pts: fn(*[pts[:, b] for b in range(dim)])
    cc = vc.cell_centres(t, n, dim)
    cells = np.concatenate([np.stack([cc[p, b].ravel() for b in range(dim)], axis=1) for p in range(L.P)])
    walls = vc.boundary_centres(L, t)
    rho, rho_wall = 1.0 / at(beta_fn, cells), 1.0 / at(beta_fn, walls)  # rho = exp(-sum x) at the centres and on the walls
    exact, F, bd = at(u_fn, cells), at(F_fn, cells), at(u_fn, walls)
    coarse = 32 if dim == 2 else 16
    # the CPU composition on the statement's beta
    beta_ref = du.faces_from_cells(L, rho, du.RECIP_MEAN, rho_wall)
    rhs_ref, _ = du.boundary_rhs_weighted(L, beta_ref, bd, F)
    x_ref, _ = vc.bicgstab(levels, vc.restrict_all(levels, beta_ref), rhs_ref, prolong_util.direct, tol=1e-12, coarse=coarse)
    # the device: rho -> beta -> coefficient -> right-hand side -> solve
    dbeta, dbd = g.new_face_vector(0), g.new_boundary_vector(0, bd)
    g.faces_from_cells(g.new_vector(0, rho), dbeta, mode=capi.FACE_RECIP_MEAN, cb=g.new_boundary_vector(0, rho_wall))
    try:
        g.set_coefficient(dbeta)
        db, dx = g.new_vector(0, F), g.new_vector(0)
        g.add_boundary_rhs_weighted(dbd, dbeta, db)
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=coarse)
        its, rr = g.bicgstab(dx, db, o, tol=1e-12, max_it=60)
        e_dev, e_ref = np.abs(dx.download() - exact).max(), np.abs(x_ref - exact).max()
        print(f"{name} {dim}d: {its} iterations, max error device {e_dev:.6e} composition {e_ref:.6e}")
        assert rr <= 1e-12 and abs(e_dev - e_ref) <= 1e-8 * e_ref
        # the projection of a random U*: f = div U*, A_b p = f, U = U* - beta (.) grad p in one pass
        Ustar = util.rand_vec(L.P * pu.face_size(n, dim), 200)
        dU, df, dp, dr, dd = g.new_face_vector(0, Ustar), g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0)
        g.divergence(dU, df)
        its, rr = g.bicgstab(dp, df, o, tol=1e-12, max_it=60)
        assert rr <= 1e-12
        g.residual(dp, df, dr)
        g.project_weighted(dU, dp, dbeta, alpha=1.0)
        g.divergence(dU, dd)
        bmax = dbeta.download().max()
        bound = dr.infNorm() + 2 * bmax * util.op_tol(L, dp.download()) + 4 * EPS * 2 * dim / L.a["h"].min() * np.abs(Ustar).max()
        print(f"{name} {dim}d projection: max|div U*| {df.infNorm():.3e} -> max|div U| {dd.infNorm():.3e}, bound {bound:.3e}")
        assert dd.infNorm() <= bound
    finally:
        g.set_coefficient(None)


# ---- refusals and state
def test_refusals():
    S, S2 = solver("2refine.bin", 0, bc_util.CHANNEL, 4, 3), solver("uniform", 1, bc_util.CHANNEL, 4, 3)
    g, g2 = S.g, S2.g
    c, c1, F, F2, F1, b, b1, i = (g.new_vector(0), g.new_vector(1), g.new_face_vector(0), g.new_face_vector(0), g.new_face_vector(1),
                                  g.new_boundary_vector(0), g.new_boundary_vector(1), g.new_iface_vector(0))
    oc, oF, ob = g2.new_vector(0), g2.new_face_vector(0), g2.new_boundary_vector(0)
    lib, NULL = capi.lib(), None
    einval = [
        # te_faces_from_cells: NULL, wrong kind, level, solver, unknown mode
        lambda: capi.check(lib.te_faces_from_cells(g.h, 0, 0, NULL, NULL, F.h)), lambda: capi.check(lib.te_faces_from_cells(g.h, 0, 0, c.h, NULL, NULL)),
        lambda: capi.check(lib.te_faces_from_cells(NULL, 0, 0, c.h, NULL, F.h)),
        lambda: g.faces_from_cells(F2, F), lambda: g.faces_from_cells(b, F), lambda: g.faces_from_cells(i, F), lambda: g.faces_from_cells(c, c),
        lambda: g.faces_from_cells(c, b), lambda: g.faces_from_cells(c, F, cb=c), lambda: g.faces_from_cells(c, F, cb=F2), lambda: g.faces_from_cells(c, F, cb=i),
        lambda: g.faces_from_cells(c1, F), lambda: g.faces_from_cells(c, F1), lambda: g.faces_from_cells(c, F, cb=b1), lambda: g.faces_from_cells(c, F, level=1),
        lambda: g.faces_from_cells(c, F, level=-1), lambda: g.faces_from_cells(c, F, level=g.num_levels),
        lambda: g.faces_from_cells(oc, F), lambda: g.faces_from_cells(c, oF), lambda: g.faces_from_cells(c, F, cb=ob),
        lambda: g.faces_from_cells(c, F, mode=3), lambda: g.faces_from_cells(c, F, mode=-1),
        # te_project_weighted: aliasing, wrong kinds, levels, solvers
        lambda: g.project_weighted(F, c, F), lambda: g.project_weighted(F, F2, F2), lambda: g.project_weighted(c, c, F), lambda: g.project_weighted(F, c, c),
        lambda: g.project_weighted(F, c, b), lambda: g.project_weighted(F, c, F2, bdata=c), lambda: g.project_weighted(F, c, F2, bdata=F),
        lambda: g.project_weighted(F1, c, F2), lambda: g.project_weighted(F, c1, F2), lambda: g.project_weighted(F, c, F1), lambda: g.project_weighted(F, c, F2, bdata=b1),
        lambda: g.project_weighted(F, c, F2, level=1), lambda: g.project_weighted(oF, c, F2), lambda: g.project_weighted(F, oc, F2), lambda: g.project_weighted(F, c, oF),
        lambda: capi.check(lib.te_project_weighted(g.h, 0, 1.0, c.h, NULL, NULL, F.h)), lambda: capi.check(lib.te_project_weighted(g.h, 0, 1.0, NULL, NULL, F2.h, F.h)),
        # te_add_boundary_rhs_weighted
        lambda: g.add_boundary_rhs_weighted(c, F, c), lambda: g.add_boundary_rhs_weighted(b, c, c), lambda: g.add_boundary_rhs_weighted(b, F, F2),
        lambda: g.add_boundary_rhs_weighted(b, F, b), lambda: g.add_boundary_rhs_weighted(b1, F, c), lambda: g.add_boundary_rhs_weighted(b, F1, c),
        lambda: g.add_boundary_rhs_weighted(b, F, c1), lambda: g.add_boundary_rhs_weighted(b, F, c, level=1), lambda: g.add_boundary_rhs_weighted(ob, F, c),
        lambda: g.add_boundary_rhs_weighted(b, oF, c), lambda: g.add_boundary_rhs_weighted(b, F, oc),
        lambda: capi.check(lib.te_add_boundary_rhs_weighted(g.h, 0, NULL, F.h, c.h)),
    ]
    for k, call in enumerate(einval):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL, k


def test_sharded_hierarchies():
    """calls 1 and 2 are refused; the fold is patch-local and runs"""
    m = util.mesh("uniform", 2)
    gs = capi.GMG(capi.Hierarchy(m, 4, rank=0, nranks=2))
    c, F, F2 = gs.new_vector(0), gs.new_face_vector(0), gs.new_face_vector(0)
    for call in (lambda: gs.faces_from_cells(c, F), lambda: gs.project_weighted(F, c, F2)):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_ESTATE and "sharded" in str(e.value)
    b = gs.new_boundary_vector(0)
    assert b.size > 0
    bd = util.rand_vec(b.size, 1)
    b.upload(bd)
    F.set(1.0)
    f = util.rand_vec(c.size, 2)
    d1, d0 = gs.new_vector(0, f), gs.new_vector(0, f)
    gs.add_boundary_rhs_weighted(b, F, d1)
    gs.add_boundary_rhs(b, d0)
    assert np.array_equal(d1.download(), d0.download()) and not np.array_equal(d0.download(), f)


@pytest.mark.parametrize("with_coefficient", [False, True], ids=["laplacian", "coefficient"])
@pytest.mark.parametrize("key", [("2refine.bin", 0, bc_util.CHANNEL, 8, 3), ("2d2ref.bin", 0, bc_util.MASKS2[0], 8, 2)], ids=["3d", "2d"])
def test_the_calls_leave_the_solver_as_it_was(key, with_coefficient):
    S = solver(*key)
    g, n, dim, L = S.g, S.n, S.dim, S.levels[0]
    d = inputs(S.key, 0)
    f = g.new_vector(0, d.f)
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)

    def cycle_sum():
        u = g.new_vector(0)
        g.cycle(o, f, u)
        g.cycle(o, f, u)
        return u.checksumLocal()

    try:
        if with_coefficient:
            g.set_coefficient(g.new_face_vector(0, positive(d.w.size, 9)))
        coef = lambda: [g_coefficient(g, l) for l in range(g.num_levels)] if with_coefficient else []
        before, coef_before = cycle_sum(), coef()
        for l in range(g.num_levels):
            e = inputs(S.key, l)
            dF, dw = g.new_face_vector(l), g.new_face_vector(l, e.w)
            g.faces_from_cells(g.new_vector(l, e.c), dF, mode=capi.FACE_HARMONIC, cb=g.new_boundary_vector(l, e.cb), level=l)
            g.project_weighted(dF, g.new_vector(l, e.p), dw, alpha=0.5, bdata=g.new_boundary_vector(l, e.bd), level=l)
            g.add_boundary_rhs_weighted(g.new_boundary_vector(l, e.bd), dw, g.new_vector(l, e.f), level=l)
        assert g.has_coefficient() == with_coefficient
        assert cycle_sum() == before
        for a, b in zip(coef(), coef_before):
            assert np.array_equal(a, b)
        # faces_from_cells right in front of an operator application: te_apply refills the ghost slots it reads
        u = g.new_vector(0, d.p)
        A0, A1 = g.new_vector(0), g.new_vector(0)
        g.apply(u, A0)
        g.faces_from_cells(g.new_vector(0, d.c), g.new_face_vector(0))
        g.apply(u, A1)
        assert A0.checksumLocal() == A1.checksumLocal()
    finally:
        g.set_coefficient(None)


def g_coefficient(g, l):
    v = g.new_face_vector(l)
    g.coefficient(l, v)
    return v.download()


def test_profile_rows_name_the_three_classes():
    S = solver("uniform", 1, bc_util.CHANNEL, 8, 3)
    g, d = S.g, inputs(S.key, 0)
    dF, dw = g.new_face_vector(0), g.new_face_vector(0, d.w)
    g.profile(True)
    g.profile_reset()
    g.faces_from_cells(g.new_vector(0, d.c), dF)
    g.project_weighted(dF, g.new_vector(0, d.p), dw)
    g.add_boundary_rhs_weighted(g.new_boundary_vector(0, d.bd), dw, g.new_vector(0))
    rows = g.profile_rows()
    g.profile(False)
    for k in ("faces_from_cells", "project_weighted"):
        assert k in rows and rows[k]["calls"] == 1 and rows[k]["cells"] == S.H.cells(0), (k, sorted(rows))
    assert rows["boundary_rhs_w"]["calls"] == 1 and rows["boundary_rhs_w"]["cells"] == d.bd.size
