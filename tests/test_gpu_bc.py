"""-m gpu: one boundary kind per side of the domain (capi.Hierarchy(neumann_sides=mask)) and boundary data on the device, against
the CPU oracle with the same mask applied per patch (tests/bc_util.py; the oracle under mixed masks is pinned to the reference's
compiled code by tests/test_bc_host.py).

Tolerances are the ones the same operations have in tests/test_gpu_parity.py (operator level: 32 eps (4 dim / h^2) |u|; sweeps:
256 eps (|u| + |f| h^2); patch solve 1e-11; restriction / prolongation bit-exact; cycle 1e-10; solve: iteration count +-1,
solution 1e-8), tests/test_gpu_init.py (1e-13 max|f|) and tests/test_gpu_schur.py (1e-8 max|u|).
Discretisation: second order means the volume-weighted L2 error falls by 4 from n = 8 to n = 16; the oracle alone gives 4.00-4.10
on these cases, a first-order boundary closure gives 2: the bound is 3.5."""
import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi, dist as tedist, problems, solver
from tests import bc_util, util
from tests.bc_util import CHANNEL, LOWER, MASKS2, MASKS3, XONLY
from tests.test_bc_host import fold_numpy

pytestmark = pytest.mark.gpu

# (mesh, n, divides, dim): one-patch coarsest levels with mixed axes, coarse/fine faces, 32^3 patches (the matrix-core solve with
# pure-Neumann, pure-Dirichlet and mixed plans side by side), a five-level tree, the 2D kernels (64^2: the half-size transforms)
MESHES = [("uniform", 16, 2, 3), ("uniform", 8, 2, 3), ("2refine.bin", 32, 0, 3), ("multi_refine.bin", 8, 0, 3),
          ("2d2ref.bin", 16, 1, 2), ("uniform", 64, 3, 2)]
CASES = [c + (mask,) for c in MESHES for mask in (MASKS3 if c[3] == 3 else MASKS2)]
# 512 patches of 32^3: the default fuse = 3 path, the case smoke() runs (the oracle's 256^3 cycle is the expensive piece: one mask)
CASES.append(("uniform", 32, 3, 3, CHANNEL))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}d-{c[4]:06b}")
def case(request):
    name, n, div, dim, mask = request.param
    orc.set_threads(16)
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    return dict(H=H, levels=levels, g=capi.GMG(H), n=n, dim=dim, mask=mask)


def test_apply_residual_and_sweeps_per_level(case):
    g = case["g"]
    for l, L in enumerate(case["levels"]):
        u = util.rand_vec(L.size, 10 + l)
        h2 = L.a["h"].min() ** 2
        f = util.rand_vec(L.size, 20 + l) / h2
        du, df, dr = g.new_vector(l, u), g.new_vector(l, f), g.new_vector(l)
        g.apply(du, dr, level=l)
        ref = orc.apply(L, u)
        tol = util.op_tol(L, u)
        assert np.abs(dr.download() - ref).max() <= tol, l
        f1 = util.rand_vec(L.size, 30 + l)
        df1 = g.new_vector(l, f1)
        g.residual(du, df1, dr, level=l)
        assert np.abs(dr.download() - (f1 - ref)).max() <= tol + 4 * util.EPS, l
        for sm, want in ((capi.SMOOTH_JACOBI, orc.jacobi(L, f, u, 0.8)), (capi.SMOOTH_RBGS, orc.patch_rbgs(L, f, u))):
            dv = g.new_vector(l, u)
            g.smooth(df, dv, level=l, smoother=sm, omega=0.8)
            assert np.abs(dv.download() - want).max() <= 256 * util.EPS * (np.abs(u).max() + np.abs(f).max() * h2), (l, sm)
        dv = g.new_vector(l, u)
        g.smooth(df, dv, level=l, smoother=capi.SMOOTH_PATCH_SOLVE)
        assert rel(dv.download(), orc.smooth(L, f, u)) <= 1e-11, l


def test_restrict_prolong_bit_exact(case):
    g, levels = case["g"], case["levels"]
    for l in range(len(levels) - 1):
        fv = util.rand_vec(levels[l].size, 40 + l)
        cv = util.rand_vec(levels[l + 1].size, 50 + l)
        dfv, dcv = g.new_vector(l, fv), g.new_vector(l + 1)
        g.restrict(dcv, dfv, fine_level=l)
        assert np.array_equal(dcv.download(), orc.restrict(levels[l], levels[l + 1], fv))
        dcv.upload(cv)
        g.interpolate(dcv, dfv, fine_level=l)
        assert np.array_equal(dfv.download(), orc.prolong_add(levels[l], levels[l + 1], cv, fv))


@pytest.mark.parametrize("smoother", [capi.SMOOTH_PATCH_SOLVE, capi.SMOOTH_RBGS], ids=["patch_solve", "rbgs"])
@pytest.mark.parametrize("cycle_type", [0, 1], ids=["V", "W"])
def test_cycle(case, smoother, cycle_type):
    g, levels = case["g"], case["levels"]
    f = util.rand_vec(levels[0].size, 70)
    want = orc.cycle(levels, orc.cycle_opts(smoother=smoother, cycle_type=cycle_type), f)
    for fuse in (0, 3):
        df, du = g.new_vector(0, f), g.new_vector(0)
        du.set(123.0)  # Cycle::apply ignores the incoming u
        g.cycle(g.default_opts(smoother=smoother, cycle_type=cycle_type, fuse=fuse), df, du)
        err = rel(du.download(), want)
        print(f"cycle mask={case['mask']:06b} smoother={smoother} type={cycle_type} fuse={fuse}: {err:.3e}")
        assert err <= 1e-10, (fuse, err)


def test_default_cycle_takes_the_fused_kernels_under_a_mask():
    """512 patches of 32^3 under the channel mask: the default cycle runs the fused kernels (what smoke() asserts for the
    all-Dirichlet domain), and fuse = 2 == fuse = 3 bit for bit"""
    m, H, levels = bc_util.setup("uniform", 32, 3, CHANNEL)
    g = capi.GMG(H)
    f = util.rand_vec(levels[0].size, 71) / levels[0].a["h"].min() ** 2
    for sm, cls in ((capi.SMOOTH_RBGS, "rbgs_resweep_prolong"), (capi.SMOOTH_PATCH_SOLVE, "patch_solve_mfma")):
        got = {}
        for fuse in (2, 3):
            df, du = g.new_vector(0, f), g.new_vector(0)
            g.profile(True)
            g.profile_reset()
            g.cycle(g.default_opts(smoother=sm, fuse=fuse), df, du)
            rows = g.profile_rows()
            g.profile(False)
            got[fuse] = du.download()
            if fuse == 3:
                assert cls in rows, sorted(rows)
        assert np.array_equal(got[2], got[3]), sm


@pytest.mark.parametrize("name,n,div,dim", [("uniform", 16, 2, 3), ("2refine.bin", 32, 0, 3), ("uniform", 32, 3, 3), ("2d2ref.bin", 16, 1, 2)])
def test_legacy_flag_and_full_masks_are_the_same_solver(name, n, div, dim):
    m = util.mesh(name, div, dim)
    allbits = (1 << 2 * dim) - 1
    for mask, flag in ((0, False), (allbits, True)):
        ga, gb = capi.GMG(capi.Hierarchy(m, n, neumann=flag)), capi.GMG(capi.Hierarchy(m, n, neumann_sides=mask))
        f = util.rand_vec(ga.hier.cells(0), 72)
        for sm in (capi.SMOOTH_PATCH_SOLVE, capi.SMOOTH_RBGS):
            out = []
            for g in (ga, gb):
                df, du = g.new_vector(0, f), g.new_vector(0)
                g.cycle(g.default_opts(smoother=sm), df, du)
                out.append(du.download())
            assert np.array_equal(out[0], out[1]), (mask, sm)
        for problem in (capi.PROBLEM_TRIG, capi.PROBLEM_GAUSS):
            fa, ea, fb, eb = ga.new_vector(0), ga.new_vector(0), gb.new_vector(0), gb.new_vector(0)
            ga.init_problem(fa, ea, problem=problem, neumann=flag)
            gb.init_problem_sides(fb, eb, problem=problem)
            assert np.array_equal(fa.download(), fb.download()) and np.array_equal(ea.download(), eb.download()), (mask, problem)


@pytest.mark.parametrize("mask", [CHANNEL, LOWER], ids=["channel", "lower"])
@pytest.mark.parametrize("name,n,div", [("uniform", 16, 2), ("2refine.bin", 8, 0), ("multi_refine.bin", 8, 0)])
def test_solve_without_mean_subtraction(name, n, div, mask):
    """a mixed domain is regular: te_bicgstab + the default cycle reaches 1e-12 on the right-hand side as it is"""
    m, H, levels = bc_util.setup(name, n, div, mask)
    assert not H.singular
    g = capi.GMG(H)
    df, de = g.new_vector(0), g.new_vector(0)
    g.init_problem_sides(df, de)
    f = df.download()
    for sm in (capi.SMOOTH_PATCH_SOLVE, capi.SMOOTH_RBGS):
        dx = g.new_vector(0)
        its, rr = g.bicgstab(dx, df, g.default_opts(smoother=sm), tol=1e-12)
        x_ref, its_ref, rr_ref = orc.bicgstab(levels, orc.cycle_opts(smoother=sm), f)
        print(f"solve {name} n={n} mask={mask:06b} smoother={sm}: its {its} (oracle {its_ref}), rr {rr:.2e}, diff {rel(dx.download(), x_ref):.2e}")
        assert rr <= 1e-12 and abs(its - its_ref) <= 1, (its, its_ref, rr)
        assert rel(dx.download(), x_ref) <= 1e-8


def l2_error(g, H, n, dx, de):
    t = H.tables(0)
    cell = np.prod(t["lengths"] / n, axis=1)
    d = (dx.download() - de.download()).reshape(len(cell), -1)
    return float(np.sqrt(np.sum((d * d).sum(axis=1) * cell)))


@pytest.mark.parametrize("mask", MASKS3, ids=lambda m: f"{m:06b}")
@pytest.mark.parametrize("name,div", [("uniform", 2), ("2refine.bin", 0), ("multi_refine.bin", 0)])
def test_second_order_with_mixed_boundary_data(name, div, mask):
    errs = {}
    for n in (8, 16):
        H = capi.Hierarchy(util.mesh(name, div), n, neumann_sides=mask)
        g = capi.GMG(H)
        df, de, dx = g.new_vector(0), g.new_vector(0), g.new_vector(0)
        g.init_problem_sides(df, de)
        its, rr = g.bicgstab(dx, df, g.default_opts(), tol=1e-12)
        assert rr <= 1e-12
        errs[n] = l2_error(g, H, n, dx, de)
    print(f"order {name} mask={mask:06b}: {errs[8]:.3e} -> {errs[16]:.3e}, ratio {errs[8] / errs[16]:.2f}")
    assert errs[8] / errs[16] >= 3.5


BD_CASES = [("uniform", 8, 2, 3, LOWER), ("2refine.bin", 16, 1, 3, CHANNEL), ("uniform", 32, 2, 3, XONLY), ("multi_refine.bin", 8, 0, 3, LOWER),
            ("2d2ref.bin", 16, 1, 2, 0b0111), ("uniform", 64, 2, 2, 0b0101)]


@pytest.mark.parametrize("name,n,div,dim,mask", BD_CASES)
def test_boundary_data_on_the_device(name, n, div, dim, mask):
    H = capi.Hierarchy(util.mesh(name, div, dim), n, neumann_sides=mask)
    g = capi.GMG(H)
    t = H.tables(0)
    nf = n ** (dim - 1)
    nb = H.num_bfaces(0)
    # (a) interior right-hand side + sampled boundary data folded on the device == te_init_problem_sides
    want, bd = g.new_vector(0), g.new_boundary_vector(0)
    assert bd.size == nb * nf
    g.init_problem_sides(want)
    g.boundary_sample(bd)
    host_bd = problems.boundary_data(t, n, mask, dim=dim)
    assert np.abs(bd.download() - host_bd).max() <= 1e-14 * 8 * max(np.abs(host_bd).max(), 1.0)
    interior = dict(t, nbr_kind=np.ones_like(t["nbr_kind"]))
    f0 = (problems.init_sides if dim == 3 else problems.init_sides_2d)(interior, n, mask)[0]
    df = g.new_vector(0, f0)
    g.add_boundary_rhs(bd, df)
    w = want.download()
    err = np.abs(df.download() - w).max()
    print(f"fold {name} n={n} mask={mask:b}: |sample + fold - init_sides| = {err:.3e}, bound {1e-13 * np.abs(w).max():.3e}")
    assert err <= 1e-13 * np.abs(w).max()
    # (b) random boundary data from the host, folded on the device, against the numpy fold: 4 ulp of the cell's largest term
    rb = util.rand_vec(nb * nf, 81)
    f1 = util.rand_vec(H.cells(0), 82)
    drb = g.new_boundary_vector(0)
    drb.upload_patches(0, rb[:nf * (nb // 2)])  # (blocks travel like patches)
    drb.upload_patches(nb // 2, rb[nf * (nb // 2):])
    assert np.array_equal(drb.download(), rb) and np.array_equal(drb.download_patches(1, 1), rb[nf:2 * nf])
    df1 = g.new_vector(0, f1)
    g.add_boundary_rhs(drb, df1)
    largest = np.abs(f1)
    want1 = fold_numpy(t, n, mask, rb, f1, dim, largest=largest)
    r_fold = (np.abs(df1.download() - want1) / (util.EPS * largest)).max()
    changed = df1.download() != f1
    inner = np.ones((n,) * dim, bool)
    inner[(slice(1, -1),) * dim] = False
    assert not changed.reshape((-1,) + (n,) * dim)[:, ~inner].any()  # the face layers only
    # (c) folding the negated data restores f
    drb.scale(-1.0)
    g.add_boundary_rhs(drb, df1)
    r_back = (np.abs(df1.download() - f1) / (util.EPS * largest)).max()
    print(f"fold {name} n={n} mask={mask:b}: random data, largest error in ulp of the cell's largest term: fold {r_fold:.2f}, fold + unfold {r_back:.2f}")
    assert r_fold <= 4 and r_back <= 4
    # (d) the two kinds of vector do not mix
    du = g.new_vector(0)
    for bad in (lambda: g.add_boundary_rhs(du, df1), lambda: g.apply(drb, du), lambda: g.apply(du, drb), lambda: g.add_boundary_rhs(drb, drb),
                lambda: g.boundary_sample(du), lambda: g.init_problem_sides(drb), lambda: du.copy(drb)):
        with pytest.raises(capi.TeError) as e:
            bad()
        assert e.value.code == capi.TE_EINVAL


SHARDED = [("uniform", 2, 8, 3, LOWER), ("2refine.bin", 1, 8, 3, CHANNEL), ("2d2ref.bin", 2, 8, 2, 0b0101)]


@pytest.mark.parametrize("nranks", [2, 3, 4, 8])
@pytest.mark.parametrize("name,divides,n,dim,mask", SHARDED)
def test_sharded_equals_single_rank_under_a_mask(nranks, name, divides, n, dim, mask, monkeypatch):
    """the three placements of tests/test_gpu_multirank.py::test_sharded_ops_equal_single_rank"""
    if nranks != 8:
        monkeypatch.setenv("TE_OVERLAP_MIN", "0")
    if nranks == 2:
        monkeypatch.setenv("TE_OVERLAP_MODE", "2")
    monkeypatch.setenv("TE_AGGLOMERATE", "0" if nranks == 4 else "16")
    monkeypatch.setenv("TE_REPLICATE", "0" if nranks == 3 else "1")
    mesh = util.mesh(name, divides, dim)
    H1 = capi.Hierarchy(mesh, n, neumann_sides=mask)
    g1 = capi.GMG(H1)
    nc, nf = n ** dim, n ** (dim - 1)
    u, f = util.rand_vec(H1.cells(0), 1), util.rand_vec(H1.cells(0), 2)
    bd = util.rand_vec(H1.num_bfaces(0) * nf, 3)
    bidx1 = H1.bface_index(0)

    def fold(g, du, df, dr, dbd):
        dr.copy(df)
        g.add_boundary_rhs(dbd, dr)

    ops = {
        "apply": lambda g, du, df, dr, dbd: g.apply(du, dr),
        "rbgs": lambda g, du, df, dr, dbd: (g.smooth(df, du, smoother=capi.SMOOTH_RBGS), dr.copy(du)),
        "jacobi": lambda g, du, df, dr, dbd: (g.smooth(df, du, smoother=capi.SMOOTH_JACOBI, omega=0.8), dr.copy(du)),
        "patch": lambda g, du, df, dr, dbd: (g.smooth(df, du, smoother=capi.SMOOTH_PATCH_SOLVE), dr.copy(du)),
        "vcycle_rbgs": lambda g, du, df, dr, dbd: g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), df, dr),
        "vcycle_patch": lambda g, du, df, dr, dbd: g.cycle(g.default_opts(smoother=capi.SMOOTH_PATCH_SOLVE), df, dr),
        "fold": fold,
    }

    def run(g, lu, lf, lbd):
        out = {}
        for k, op in ops.items():
            du, df, dr = g.new_vector(0, lu), g.new_vector(0, lf), g.new_vector(0)
            dbd = g.new_boundary_vector(0, lbd if lbd.size else None)
            op(g, du, df, dr, dbd)
            out[k] = dr.download()
            if k == "vcycle_rbgs":
                out["checksum"] = dr.checksumLocal()
        return out

    want = run(g1, u, f, bd)

    fab = tedist.LocalFabric(nranks)
    hs = [capi.Hierarchy(mesh, n, rank=r, nranks=nranks, neumann_sides=mask) for r in range(nranks)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)

    def per_rank(r):
        H, idx = hs[r], hs[r].l2g(0)
        blocks = [bidx1[gp, s] for gp in idx for s in range(2 * dim) if bidx1[gp, s] >= 0]  # this rank's faces, (patch, side) order
        lbd = bd.reshape(-1, nf)[blocks].ravel() if blocks else np.zeros(0)
        assert H.num_bfaces(0) == len(blocks)
        return run(gs[r], u.reshape(-1, nc)[idx].ravel(), f.reshape(-1, nc)[idx].ravel(), lbd)

    outs = fab.run(per_rank)
    for k in ops:
        full = np.zeros_like(u)
        for r in range(nranks):
            idx = hs[r].l2g(0)
            full.reshape(-1, nc)[idx] = outs[r][k].reshape(len(idx), nc)
        assert np.array_equal(full, want[k]), (k, np.abs(full - want[k]).max())
    assert sum(o["checksum"] for o in outs) % (1 << 64) == want["checksum"]


def test_ranks_with_different_masks_are_told_so():
    mesh = util.mesh("uniform", 2)
    fab = tedist.LocalFabric(2)
    hs = [capi.Hierarchy(mesh, 8, rank=r, nranks=2, neumann_sides=(CHANNEL if r == 0 else LOWER)) for r in range(2)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)
        g.set_option("TE_NO_VERIFY", "1")

    def per_rank(r):
        g = gs[r]
        try:
            g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), g.new_vector(0), g.new_vector(0))
        except capi.TeError as e:
            return e.code, str(e)
        return 0, "no error"

    msgs = fab.run(per_rank)
    assert all(c == capi.TE_ESTATE and "neumann_sides" in m and "different hierarchies" in m for c, m in msgs), msgs


@pytest.mark.parametrize("name,div,n,dim,mask", [("uniform", 3, 32, 3, CHANNEL), ("2refine.bin", 1, 32, 3, CHANNEL), ("2d2ref.bin", 0, 64, 2, 0b0111)],
                         ids=["256cube-32", "2refine-div1-32", "2d2ref-64"])
def test_schur_route_under_the_channel_mask(name, div, n, dim, mask):
    H = capi.Hierarchy(util.mesh(name, div, dim), n, neumann_sides=mask)
    g = capi.GMG(H)
    df = g.new_vector(0)
    g.init_problem_sides(df)
    dw = g.new_vector(0)
    its, rr = g.bicgstab(dw, df, g.default_opts(), tol=1e-12)
    assert rr <= 1e-12
    want = dw.download()
    for prec in (None, "cheb"):
        du = g.new_vector(0)
        its, rr, gamma = solver.schur_solve(g, df, du, prec=prec, tol=1e-12)
        assert its > 0 and rr <= 1e-12, (prec, its, rr)
        assert np.abs(du.download() - want).max() <= 1e-8 * np.abs(want).max(), prec
    # the faces-only form of T and the full solve (TE_SCHUR_FULL): the same bits, whichever of the two the level's plans allow
    x = util.rand_vec(H.num_ifaces(0) * n ** (dim - 1), 17)
    dx, got = g.new_iface_vector(0, x), {}
    for full in (None, "1"):
        g.set_option("TE_SCHUR_FULL", full)
        dy = g.new_iface_vector(0)
        g.schur_apply(dx, dy)
        got[full] = dy.download()
    g.set_option("TE_SCHUR_FULL", None)
    assert np.array_equal(got[None], got["1"])
