"""-m gpu: te_gradient, te_divergence and te_project on face vectors (include/te_hip.h) against the numpy statement of
tests/projection_util.py, which tests/test_projection_host.py pins to the reference's compiled operator.

Bounds (none of them comes from what the kernels give):
  gradient      32 eps (5 / h_min) max(|u|, |g|): a few ulps of sum |coef| |u|; 5 / h is the largest coefficient sum, on the fine side
                of a coarse/fine face (2 / h (1 + 14 / 12 + 4 / 12)); Neumann faces carry g_n bit for bit
  div(grad u)   against te_apply(u) - b: util.op_tol(u) plus the same expression in |g| (b = the fold of the boundary data)
  divergence    32 eps (2 dim / h_min) max|U|; alpha scales the result as exactly one multiplication
  project       2 eps (|U| + |alpha G|) per entry against U - alpha G
  shared faces, sharded runs: bit for bit
  end to end    max|div U| <= max|f - A p| + 2 op_tol(p) + 4 eps (2 dim / h_min) max|U*|
"""
import glob
import os

import numpy as np
import pytest

from pressurepoissonsolver_amd import capi, dist as tedist
from tests import bc_util, projection_util as pu, util
from tests.bc_util import CHANNEL, LOWER, MASKS2, MASKS3

pytestmark = pytest.mark.gpu

# the meshes of tests/test_gpu_bc.py plus 4^3 / 4^2 patches (the smallest size te_gmg_create accepts)
MESHES = [("uniform", 16, 2, 3), ("uniform", 8, 2, 3), ("2refine.bin", 32, 0, 3), ("multi_refine.bin", 8, 0, 3),
          ("2d2ref.bin", 16, 1, 2), ("uniform", 64, 3, 2), ("uniform", 4, 2, 3), ("2refine.bin", 4, 0, 3), ("2d2ref.bin", 4, 1, 2)]


def masks_of(dim):
    return (0, (1 << 2 * dim) - 1) + (MASKS3 if dim == 3 else MASKS2)  # all-Dirichlet, all-Neumann, mixed


CASES = [c + (mask,) for c in MESHES for mask in masks_of(c[3])]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}d-{c[4]:06b}")
def case(request):
    name, n, div, dim, mask = request.param
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    return dict(H=H, levels=levels, g=capi.GMG(H), n=n, dim=dim, mask=mask)


def boundary_data(L, seed):
    return util.rand_vec(pu.num_bfaces(L) * L.nf, seed)


def face(lo, hi, p, s, dim):
    """the values on side s of patch p"""
    a = s >> 1
    return hi[p, a] if s & 1 else np.take(lo[p, a], 0, axis=dim - 1 - a)


def test_gradient_against_the_numpy_statement(case):
    g, n, dim = case["g"], case["n"], case["dim"]
    for l, L in enumerate(case["levels"]):
        assert case["H"].num_bfaces(l) == pu.num_bfaces(L)
        u = util.rand_vec(L.size, 100 + l)
        du, dG = g.new_vector(l, u), g.new_face_vector(l)
        assert dG.size == L.P * pu.face_size(n, dim)
        for bd in (None, boundary_data(L, 110 + l)):
            dbd = g.new_boundary_vector(l, bd) if bd is not None else None
            g.gradient(du, dG, bdata=dbd, level=l)
            lo, hi = pu.unpack(dG.download(), n, dim)
            rlo, rhi = pu.level_grad(L, u, bd)
            err, tol = max(np.abs(lo - rlo).max(), np.abs(hi - rhi).max()), pu.grad_tol(L, u, bd)
            print(f"gradient level {l} bdata={bd is not None}: {err / tol:.3f} of the bound")
            assert err <= tol, (l, bd is not None)
            kind, neu = L.a["nbr_kind"], L.a["neumann"]
            for p in range(L.P):
                for s in range(2 * dim):
                    if kind[p, s] == 0 and (neu[p] >> s) & 1:  # a Neumann face carries its datum itself
                        assert np.array_equal(face(lo, hi, p, s, dim), face(rlo, rhi, p, s, dim)), (l, p, s)


def test_divergence_of_the_gradient_is_the_operator(case):
    g, n, dim = case["g"], case["n"], case["dim"]
    for l, L in enumerate(case["levels"]):
        u = util.rand_vec(L.size, 120 + l)
        du, dG, dd, dA = g.new_vector(l, u), g.new_face_vector(l), g.new_vector(l), g.new_vector(l)
        g.apply(du, dA, level=l)
        A = dA.download()
        for bd in (None, boundary_data(L, 130 + l)):
            tol = util.op_tol(L, u)
            b = np.zeros_like(u)
            dbd = None
            if bd is not None:
                dbd, db = g.new_boundary_vector(l, bd), g.new_vector(l)
                g.add_boundary_rhs(dbd, db, level=l)
                b = db.download()
                tol += util.op_tol(L, bd)
            g.gradient(du, dG, bdata=dbd, level=l)
            g.divergence(dG, dd, level=l)
            err = np.abs(dd.download() - (A - b)).max()
            print(f"div grad level {l} bdata={bd is not None}: {err / tol:.3f} of the bound")
            assert err <= tol, (l, bd is not None)


def test_divergence_against_numpy_and_alpha_is_one_multiplication(case):
    g, n, dim = case["g"], case["n"], case["dim"]
    for l, L in enumerate(case["levels"]):
        U = util.rand_vec(L.P * pu.face_size(n, dim), 140 + l)
        dU, d1, d2 = g.new_face_vector(l, U), g.new_vector(l), g.new_vector(l)
        g.divergence(dU, d1, level=l)
        got = d1.download()
        assert np.abs(got - pu.level_div(L, *pu.unpack(U, n, dim))).max() <= pu.div_tol(L, U), l
        g.divergence(dU, d2, alpha=-0.37, level=l)
        assert np.array_equal(d2.download(), -0.37 * got), l


def test_project_is_the_fused_update(case):
    g, n, dim = case["g"], case["n"], case["dim"]
    alpha = 0.37
    for l, L in enumerate(case["levels"]):
        U, p = util.rand_vec(L.P * pu.face_size(n, dim), 150 + l), util.rand_vec(L.size, 160 + l)
        bd = boundary_data(L, 170 + l)
        for b in (None, bd):
            dbd = g.new_boundary_vector(l, b) if b is not None else None
            dU, dG, dp = g.new_face_vector(l, U), g.new_face_vector(l), g.new_vector(l, p)
            g.gradient(dp, dG, bdata=dbd, level=l)
            g.project(dU, dp, alpha=alpha, bdata=dbd, level=l)
            G = dG.download()
            assert (np.abs(dU.download() - (U - alpha * G)) <= 2 * util.EPS * (np.abs(U) + np.abs(alpha * G))).all(), l


def test_same_level_faces_get_the_same_bits_in_both_copies(case):
    """a single-valued velocity stays single-valued: gradient, and project on a single-valued U"""
    g, n, dim = case["g"], case["n"], case["dim"]
    for l, L in enumerate(case["levels"]):
        kind, nbr = L.a["nbr_kind"], L.a["nbr"]
        pairs = [(p, a, int(nbr[p, 2 * a + 1, 0])) for p in range(L.P) for a in range(dim) if kind[p, 2 * a + 1] == 1]
        u = util.rand_vec(L.size, 180 + l)
        du, dG = g.new_vector(l, u), g.new_face_vector(l)
        g.gradient(du, dG, level=l)
        lo, hi = pu.unpack(dG.download(), n, dim)
        for p, a, q in pairs:
            assert np.array_equal(hi[p, a], np.take(lo[q, a], 0, axis=dim - 1 - a)), (l, p, a)
        Ulo, Uhi = pu.unpack(util.rand_vec(L.P * pu.face_size(n, dim), 190 + l), n, dim)
        for p, a, q in pairs:  # make U single-valued on the same-level faces
            sl = [slice(None)] * dim
            sl[dim - 1 - a] = 0
            Ulo[q, a][tuple(sl)] = Uhi[p, a]
        dU = g.new_face_vector(l, pu.pack(Ulo, Uhi))
        g.project(dU, du, alpha=0.61, level=l)
        lo, hi = pu.unpack(dU.download(), n, dim)
        for p, a, q in pairs:
            assert np.array_equal(hi[p, a], np.take(lo[q, a], 0, axis=dim - 1 - a)), (l, p, a)


FIXTURES = sorted(glob.glob(os.path.join(util.GOLDEN, "ref_*_n*.npz")))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def test_divergence_of_the_gradient_against_the_reference_apply(path):
    """golden `u` -> te_gradient -> te_divergence against the reference's compiled SchurHelper::apply (golden `apply`), vectors
    keyed by patch id as in tests/test_gpu_direct_parity.py"""
    d = dict(np.load(path))
    dim, n, neu = int(d["dim"]), int(d["n"]), bool(int(d["neumann"]))
    m, H, levels = util.setup(str(d["mesh"]), n, 0, neumann=neu, dim=dim)
    g = capi.GMG(H)
    pos = {int(i): k for k, i in enumerate(d["t_id"])}
    perm = np.array([pos[int(i)] for i in H.tables(0)["id"]])
    mine = lambda v: np.ascontiguousarray(v.reshape(-1, n ** dim)[perm]).ravel()
    du, dG, dd = g.new_vector(0, mine(d["u"])), g.new_face_vector(0), g.new_vector(0)
    g.gradient(du, dG)
    g.divergence(dG, dd)
    assert np.abs(dd.download() - mine(d["apply"])).max() <= util.op_tol(levels[0], d["u"])


SHARDED = [("uniform", 2, 8, 3, LOWER), ("2refine.bin", 1, 8, 3, CHANNEL), ("2d2ref.bin", 2, 8, 2, 0b0101)]


@pytest.mark.parametrize("nranks", [2, 3, 4, 8])
@pytest.mark.parametrize("name,divides,n,dim,mask", SHARDED)
def test_sharded_equals_single_rank(nranks, name, divides, n, dim, mask, monkeypatch):
    """the placements of tests/test_gpu_bc.py::test_sharded_equals_single_rank_under_a_mask"""
    if nranks != 8:
        monkeypatch.setenv("TE_OVERLAP_MIN", "0")
    if nranks == 2:
        monkeypatch.setenv("TE_OVERLAP_MODE", "2")
    monkeypatch.setenv("TE_AGGLOMERATE", "0" if nranks == 4 else "16")
    monkeypatch.setenv("TE_REPLICATE", "0" if nranks == 3 else "1")
    mesh = util.mesh(name, divides, dim)
    H1 = capi.Hierarchy(mesh, n, neumann_sides=mask)
    g1 = capi.GMG(H1)
    nc, nf, fs = n ** dim, n ** (dim - 1), pu.face_size(n, dim)
    P = H1.sizes(0)[0]
    u, U = util.rand_vec(P * nc, 1), util.rand_vec(P * fs, 2)
    bd = util.rand_vec(H1.num_bfaces(0) * nf, 3)
    bidx1 = H1.bface_index(0)

    def run(g, lu, lU, lbd):
        du, dU, dG, dd = g.new_vector(0, lu), g.new_face_vector(0, lU), g.new_face_vector(0), g.new_vector(0)
        dbd = g.new_boundary_vector(0, lbd if lbd.size else None)
        out = {}
        g.gradient(du, dG, bdata=dbd)
        out["gradient"], out["gradient_sum"] = dG.download(), dG.checksumLocal()
        g.divergence(dU, dd, alpha=1.5)
        out["divergence"], out["divergence_sum"] = dd.download(), dd.checksumLocal()
        g.project(dU, du, alpha=0.25, bdata=dbd)
        out["project"], out["project_sum"] = dU.download(), dU.checksumLocal()
        return out

    want = run(g1, u, U, bd)
    fab = tedist.LocalFabric(nranks)
    hs = [capi.Hierarchy(mesh, n, rank=r, nranks=nranks, neumann_sides=mask) for r in range(nranks)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)

    def per_rank(r):
        idx = hs[r].l2g(0)
        blocks = [bidx1[gp, s] for gp in idx for s in range(2 * dim) if bidx1[gp, s] >= 0]
        lbd = bd.reshape(-1, nf)[blocks].ravel() if blocks else np.zeros(0)
        return run(gs[r], u.reshape(-1, nc)[idx].ravel(), U.reshape(-1, fs)[idx].ravel(), lbd)

    outs = fab.run(per_rank)
    for k, width in (("gradient", fs), ("divergence", nc), ("project", fs)):
        full = np.zeros_like(want[k])
        for r in range(nranks):
            idx = hs[r].l2g(0)
            full.reshape(-1, width)[idx] = outs[r][k].reshape(len(idx), width)
        assert np.array_equal(full, want[k]), (k, np.abs(full - want[k]).max())
        assert sum(o[k + "_sum"] for o in outs) % (1 << 64) == want[k + "_sum"], k


def test_vector_kinds_do_not_mix():
    m, H, levels = bc_util.setup("2refine.bin", 8, 0, LOWER)
    g = capi.GMG(H)
    n, dim = 8, 3
    du, dv = g.new_vector(0), g.new_vector(0)
    dF, dF2, dF1 = g.new_face_vector(0), g.new_face_vector(0), g.new_face_vector(1)
    db, di = g.new_boundary_vector(0), g.new_iface_vector(0)
    bad = [lambda: g.gradient(dF, dF2), lambda: g.gradient(du, dv), lambda: g.gradient(du, db), lambda: g.gradient(du, di),
           lambda: g.gradient(du, dF, bdata=dv), lambda: g.gradient(du, dF, bdata=dF2), lambda: g.gradient(du, dF, bdata=di),
           lambda: g.gradient(du, dF1), lambda: g.gradient(du, dF, level=1),
           lambda: g.divergence(du, dv), lambda: g.divergence(dF, dF2), lambda: g.divergence(db, du), lambda: g.divergence(dF, db),
           lambda: g.divergence(dF1, du),
           lambda: g.project(du, dv), lambda: g.project(dF, dF2), lambda: g.project(db, du), lambda: g.project(dF, du, bdata=dF2),
           lambda: g.project(dF1, du),
           # the domain operators and the other kinds' calls refuse a face vector
           lambda: g.apply(dF, du), lambda: g.apply(du, dF), lambda: g.residual(du, dv, dF), lambda: g.smooth(dF, du),
           lambda: g.cycle(g.default_opts(), dF, du), lambda: g.bicgstab(dF, du), lambda: g.add_boundary_rhs(dF, du),
           lambda: g.add_boundary_rhs(db, dF), lambda: g.integrate(dF), lambda: du.copy(dF), lambda: dF.copy(du), lambda: dF.add(db),
           lambda: dF.dot(du), lambda: dF.copy(dF1)]
    for k, f in enumerate(bad):
        with pytest.raises(capi.TeError) as e:
            f()
        assert e.value.code == capi.TE_EINVAL, k
    # a face vector passes through the BLAS-1 calls, the checksum and the per-patch transfers
    fs = pu.face_size(n, dim)
    a, b = util.rand_vec(dF.size, 7), util.rand_vec(dF.size, 8)
    dF.upload_patches(0, a[:2 * fs])
    dF.upload_patches(2, a[2 * fs:])
    assert np.array_equal(dF.download(), a) and np.array_equal(dF.download_patches(1, 1), a[fs:2 * fs])
    dF2.upload(b)
    dF.addScaled(2.0, dF2)
    dF.scale(0.5)
    want = (a + 2.0 * b) * 0.5
    assert np.abs(dF.download() - want).max() <= 4 * util.EPS * np.abs(want).max()
    assert abs(dF.dot(dF2) - want @ b) <= 1e-12 * np.abs(want @ b) + 1e-12
    assert dF.infNorm() == np.abs(dF.download()).max()
    dF2.copy(dF)
    assert dF2.checksumLocal() == dF.checksumLocal() == int(dF.download().view(np.uint64).sum(dtype=np.uint64))


@pytest.mark.parametrize("mask", [CHANNEL, LOWER, 0], ids=["channel", "lower", "dirichlet"])
@pytest.mark.parametrize("name,n,div", [("uniform", 16, 2), ("2refine.bin", 8, 0), ("multi_refine.bin", 8, 0)])
def test_projected_field_is_divergence_free_as_far_as_the_solve_went(name, n, div, mask):
    m, H, levels = bc_util.setup(name, n, div, mask)
    g, L, dim = capi.GMG(H), levels[0], 3
    Ustar = util.rand_vec(L.P * pu.face_size(n, dim), 200)
    dU, df, dp, dr, dd = g.new_face_vector(0, Ustar), g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.divergence(dU, df)
    its, rr = g.bicgstab(dp, df, g.default_opts(), tol=1e-12)
    assert rr <= 1e-12
    g.residual(dp, df, dr)
    g.project(dU, dp)
    g.divergence(dU, dd)
    got = dd.infNorm()
    bound = dr.infNorm() + 2 * util.op_tol(L, dp.download()) + 4 * util.EPS * 2 * dim / L.a["h"].min() * np.abs(Ustar).max()
    print(f"projection {name} n={n} mask={mask:06b}: {its} iterations, max|div U*| {df.infNorm():.3e} -> max|div U| {got:.3e}, bound {bound:.3e}")
    assert got <= bound


def test_full_size_on_the_device():
    """512^3 in 32^3 patches, compared on the device (no 1 GiB downloads): div(grad u) - te_apply(u) within the operator-level
    tolerance, and the profile rows show the three new kernel classes"""
    n, dim = 32, 3
    H = capi.Hierarchy(util.mesh("uniform", 4), n)
    g = capi.GMG(H)
    du, dA, dd = g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.init_problem(du, problem=capi.PROBLEM_RANDOM)  # u ~ U(-1, 1), filled on the device
    dG = g.new_face_vector(0)
    g.profile(True)
    g.profile_reset()
    g.gradient(du, dG)
    g.divergence(dG, dd)
    g.apply(du, dA)
    dd.addScaled(-1.0, dA)
    err = dd.infNorm()
    hmin = 1.0 / (16 * n)
    tol = 32 * util.EPS * 4 * dim / hmin ** 2 * du.infNorm()  # util.op_tol
    g.project(dG, du, alpha=1.0)  # G - grad u: what is left is rounding
    left = dG.infNorm()
    rows = g.profile_rows()
    g.profile(False)
    print(f"512^3: |div grad u - A u| = {err:.3e} ({err / tol:.3f} of op_tol), |G - grad u| after project = {left:.3e}, "
          + ", ".join(f"{k} {rows[k]['ms']:.3f} ms" for k in ("gradient", "divergence", "project", "stencil_apply") if k in rows))
    assert err <= tol
    assert left <= 2 * util.EPS * 2 * 2 / hmin * du.infNorm()  # 2 eps (|U| + |alpha G|), |G| <= 2 max|u| / h
    for k in ("gradient", "divergence", "project"):
        assert k in rows and rows[k]["calls"] >= 1 and rows[k]["cells"] == H.cells(0) * rows[k]["calls"], (k, sorted(rows))
