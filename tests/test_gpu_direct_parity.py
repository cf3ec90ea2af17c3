"""-m gpu: parity of the path that is BENCHMARKED, checked directly.

(a) Default options (te_cycle_opts_default: fuse = 3) at the production patch size n = 32 on levels with >= 256
    patches -- the fused kernels bench.py times (k_rbgs_zero_resid3d, k_rbgs_resweep_prolong3d, k_restrict_fixup3d;
    k_ps_sym + the interface-only residual for the reference smoother) -- against the CPU oracle's V-cycle and
    BiCGStab on the same inputs, at BASELINE.json's full sizes:
      C2  256^3 uniform, 512 patches of 32^3            C3  512^3 uniform, 4096 patches (the headline config)
      C4  2refine.bin --divide 2, 960 patches of 32^3   C5  4096^2 uniform, 4096 patches of 64^2 (2D)
    Every test asserts from the library's own kernel-class counters that the fused kernels really ran.
    Tolerances: V-cycle 1e-10 relative 2-norm (as tests/test_gpu_parity.py); BiCGStab: same iteration count +-1,
    1e-8 on the solution.
(b) HIP output against the reference's OWN numbers: tests/golden/ref_*.npz were written by the reference's compiled
    StarPatchOp / TriLinInterp / BilinearInterpolator / Vector / BiCGStab (oracle/gen_golden.py); vectors are keyed
    by patch id. Where oracle/_ref/libte_ref.so travelled with the snapshot (it needs no reference tree), the same
    comparisons also run live against the reference's code on fresh inputs.
"""
import glob
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import refslice
from pressurepoissonsolver_amd import capi, problems
from tests import util

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---------------------------------------------------------------------------------------------- (a)
FULL = {
    "C2-256^3": dict(mesh="uniform", n=32, div=3, dim=3, patches=512),
    "C3-512^3": dict(mesh="uniform", n=32, div=4, dim=3, patches=4096),
    "C4-2refine-div2": dict(mesh="2refine.bin", n=32, div=2, dim=3, patches=960),
    "C5-4096^2": dict(mesh="uniform", n=64, div=6, dim=2, patches=4096),
    "256^3-in-16^3": dict(mesh="uniform", n=16, div=4, dim=3, patches=4096),  # the 16^3 kernels (k_ps16) at depth
}
# kernel classes (te_gmg_profile_rows) that prove which path a default-option cycle took
FUSED_RBGS_3D = ("rbgs_zero_resid_restrict_faces", "rbgs_resweep_prolong", "restrict_fixup")
FUSED_RBGS_REFINED = ("rbgs_zero_resid_restrict_faces", "rbgs_resweep_prolong", "restrict_fixup", "cf_ghost")
FUSED_PS_3D = ("patch_solve_mfma", "restrict_fixup")
FUSED_2D = ("rbgs_zero_resid_restrict_faces", "rbgs_resweep_prolong", "restrict_fixup")


@pytest.fixture(scope="module", params=list(FULL), ids=list(FULL))
def full(request):
    c = FULL[request.param]
    m, H, levels = util.setup(c["mesh"], c["n"], c["div"], dim=c["dim"])
    assert levels[0].P == c["patches"]
    orc.set_threads(min(os.cpu_count() or 1, 16))
    g = capi.GMG(H)
    f = problems.random_rhs(H.tables(0)["id"], c["n"] ** c["dim"])
    return dict(name=request.param, H=H, levels=levels, g=g, f=f, **c)


def run_default_cycle(g, f, smoother):
    o = g.default_opts(smoother=smoother)
    assert o.fuse == 3 and o.pre_sweeps == 1 and o.post_sweeps == 1 and o.cycle_type == 0  # bench.py's options
    df, du = g.new_vector(0, f), g.new_vector(0)
    du.set(7.0)  # Cycle::apply ignores the incoming u (Cycle.h:118)
    g.profile(True)
    g.profile_reset()
    g.cycle(o, df, du)
    rows = g.profile_rows()
    g.profile(False)
    return du.download(), rows


@pytest.mark.parametrize("smoother", [capi.SMOOTH_RBGS, capi.SMOOTH_PATCH_SOLVE], ids=["rbgs", "patch_solve"])
def test_default_cycle_against_oracle_at_full_size(full, smoother):
    g, levels, f = full["g"], full["levels"], full["f"]
    got, rows = run_default_cycle(g, f, smoother)
    if full["dim"] == 3 and smoother == capi.SMOOTH_RBGS:
        need = FUSED_RBGS_REFINED if full["mesh"] != "uniform" else FUSED_RBGS_3D
    elif full["dim"] == 3:
        need = FUSED_PS_3D
    else:
        need = FUSED_2D if smoother == capi.SMOOTH_RBGS else ("patch_solve_mfma",)  # (64^2 patches: k_patch_solve2d_mfma)
    for k in need:
        assert k in rows and rows[k]["calls"] >= 1, (k, sorted(rows))
    if full["mesh"] == "uniform" and full["dim"] == 3 and smoother == capi.SMOOTH_RBGS:
        # nothing but the fused kernels touches the levels with >= 256 patches
        # (a level below another fused level reads its right-hand side with the exported ghost terms: classes *_fcorr)
        big = sum(L.P >= 256 for L in levels[:-1])
        calls = lambda k: rows.get(k, {"calls": 0})["calls"] + rows.get(k + "_fcorr", {"calls": 0})["calls"]  # noqa: E731
        assert calls("rbgs_resweep_prolong") == big and calls("rbgs_zero_resid_restrict_faces") == big
        assert ("fcorr_gather" in rows) == (big >= 2)
        assert "stencil_rbgs" not in rows and "resid_restrict" not in rows and "prolong_add" not in rows
    want = orc.cycle(levels, orc.cycle_opts(smoother=smoother), f)
    assert rel(got, want) <= 1e-10
    # and the cycle does what a cycle must: the reference smoother contracts the residual ~0.05 (3D) / ~0.13 (2D),
    # RB-GS ~0.18 (3D)
    r = f - orc.apply(levels[0], got)
    assert np.linalg.norm(r) <= (0.2 if smoother == capi.SMOOTH_PATCH_SOLVE else 0.35) * np.linalg.norm(f)


OTHER_SHAPES = {  # cycles other than bench.py's V(1,1), at C2's full size (256^3, 512 patches): options for both sides
    "w-cycle-rbgs": dict(smoother=capi.SMOOTH_RBGS, cycle_type=1),
    "v22-rbgs": dict(smoother=capi.SMOOTH_RBGS, pre_sweeps=2, post_sweeps=2),
    "v11-jacobi": dict(smoother=capi.SMOOTH_JACOBI, omega=0.8),
    "w-cycle-patch-solve": dict(smoother=capi.SMOOTH_PATCH_SOLVE, cycle_type=1),
    "v11-rbgs-relaxed-coarse": dict(smoother=capi.SMOOTH_RBGS, exact_coarse=0, coarse_sweeps=3),
}


@pytest.mark.parametrize("shape", list(OTHER_SHAPES))
@pytest.mark.parametrize("neumann", [False, True], ids=["dirichlet", "neumann"])
def test_other_cycle_shapes_against_oracle_at_c2_size(shape, neumann):
    """W-cycles (WCycle.h:45-68), V(2,2), weighted Jacobi and a relaxed coarsest level on 256^3 with default fusion, Dirichlet
    and Neumann physical boundaries (the Neumann patch solve splits the level between k_ps_sym and k_ps_fused)."""
    kw = OTHER_SHAPES[shape]
    m, H, levels = util.setup("uniform", 32, 3, neumann=neumann)
    assert levels[0].P == 512
    orc.set_threads(min(os.cpu_count() or 1, 16))
    g = capi.GMG(H)
    f = problems.random_rhs(H.tables(0)["id"], 32 ** 3)
    if neumann:
        f -= f.mean()  # (uniform cells: a compatible right-hand side)
    df, du = g.new_vector(0, f), g.new_vector(0)
    g.cycle(g.default_opts(**kw), df, du)
    names = dict(pre_sweeps="pre", post_sweeps="post", coarse_sweeps="coarse")
    want = orc.cycle(levels, orc.cycle_opts(**{names.get(k, k): v for k, v in kw.items()}), f)
    assert rel(du.download(), want) <= 1e-10


def solve_fixture(tag, name):
    """tests/golden/<tag>_solve_<smoother>.npz: the oracle's BiCGStab + GMG solve of the trig problem, run once in the build
    container by oracle/gen_c3_solve.py (iteration count, residual, norms, 4096 sampled entries keyed by patch id and cell)"""
    return dict(np.load(os.path.join(util.GOLDEN, f"{tag}_solve_{name}.npz")))


def against_fixture(x, ids, nc, fx, tol):
    """relative 2-norm difference on the fixture's samples, and the relative difference of the norms of the whole vectors"""
    pos = {int(i): k for k, i in enumerate(ids)}
    rows = np.array([pos[int(i)] for i in fx["patch_id"]])
    got = x.reshape(-1, nc)[rows, fx["cell"]]
    assert rel(got, fx["value"]) <= tol, rel(got, fx["value"])
    assert abs(np.linalg.norm(x) - float(fx["x_norm2"])) <= tol * float(fx["x_norm2"])


@pytest.mark.parametrize("smoother", [capi.SMOOTH_RBGS, capi.SMOOTH_PATCH_SOLVE], ids=["rbgs", "patch_solve"])
def test_default_bicgstab_against_oracle_at_full_size(full, smoother):
    """te_bicgstab + default-option V-cycle (the call of apps/3d/steady.cpp:519-524 over BiCGStab.h:45-106) against the oracle's
    solve with the SAME smoother: iteration count +-1, 1e-8 on the solution, the same discretisation error. C3 (512^3, the
    headline size): against the committed fixture of the oracle's solve (3 min of host time per smoother, run once)."""
    g, levels, H = full["g"], full["levels"], full["H"]
    init = problems.init_dirichlet if full["dim"] == 3 else problems.init_dirichlet_2d
    b, exact = init(H.tables(0), full["n"])
    db, dx = g.new_vector(0, b), g.new_vector(0)
    its, rr = g.bicgstab(dx, db, g.default_opts(smoother=smoother))
    x = dx.download()
    name = "rbgs" if smoother == capi.SMOOTH_RBGS else "patch_solve"
    tag = {"C3-512^3": "c3", "C2-256^3": "c2", "C4-2refine-div2": "c4", "256^3-in-16^3": "d16"}.get(full["name"])
    if tag:
        # the oracle's solve from its committed fixture (oracle/gen_c3_solve.py, run once in the build container: minutes of host time
        # per configuration that every GPU test run used to repeat). C2 with RB-GS goes both ways: the fixture format is itself checked
        # against the live oracle below
        fx = solve_fixture(tag, name)
        assert int(fx["n"]) == full["n"] and int(fx["smoother"]) == smoother
        assert rr <= 1e-12 and float(fx["rr"]) <= 1e-12 and abs(its - int(fx["its"])) <= 1
        against_fixture(x, H.tables(0)["id"], full["n"] ** 3, fx, 1e-8)
        e = rel(x, exact)
        assert abs(e - float(fx["err_rel"])) <= 1e-3 * float(fx["err_rel"])
        if not (tag == "c2" and smoother == capi.SMOOTH_RBGS):
            return
    x_ref, its_ref, rr_ref = orc.bicgstab(levels, orc.cycle_opts(smoother=smoother), b)
    assert rr <= 1e-12 and rr_ref <= 1e-12 and abs(its - its_ref) <= 1
    assert rel(x, x_ref) <= 1e-8
    e, e_ref = rel(x, exact), rel(x_ref, exact)
    assert abs(e - e_ref) <= 1e-3 * e_ref  # the same discretisation error against the analytic solution
    if full["name"] == "C2-256^3":  # the fixture says what the live oracle says
        fx = solve_fixture("c2", name)
        assert int(fx["its"]) == its_ref
        against_fixture(x_ref, H.tables(0)["id"], full["n"] ** 3, fx, 1e-13)


def test_headline_solve_matches_reference_smoother_solve(full):
    """BASELINE.json's sentence, literally: "results must match the reference CPU GMG solve on the same RHS to a stated
    floating-point tolerance" -- the HEADLINE path (HIP BiCGStab preconditioned with the patch-local RB-GS V-cycle, default
    options) against the CPU solve with the REFERENCE's smoother (oracle BiCGStab + block-Jacobi patch-solve V-cycle,
    FFTBlockJacobiSmoother.h:55-58) on the drivers' trig right-hand side (apps/3d/steady.cpp:253-265). Two different
    preconditioners, one linear system A x = b, both converged to 1e-12: the solutions agree to 1e-8 (SURVEY Appendix A,
    solve-level parity) and carry the same discretisation error. C2 live, C3 through the committed fixture."""
    if full["dim"] != 3 or full["mesh"] != "uniform" or full["n"] != 32:
        pytest.skip("stated for the uniform 3D configurations (C2, C3)")
    g, levels, H = full["g"], full["levels"], full["H"]
    b, exact = problems.init_dirichlet(H.tables(0), full["n"])
    db, dx = g.new_vector(0, b), g.new_vector(0)
    its, rr = g.bicgstab(dx, db, g.default_opts(smoother=capi.SMOOTH_RBGS))
    x = dx.download()
    assert rr <= 1e-12
    fx = solve_fixture("c3" if full["name"].startswith("C3") else "c2", "patch_solve")
    assert int(fx["smoother"]) == capi.SMOOTH_PATCH_SOLVE and float(fx["rr"]) <= 1e-12
    against_fixture(x, H.tables(0)["id"], full["n"] ** 3, fx, 1e-8)
    e = rel(x, exact)
    assert abs(e - float(fx["err_rel"])) <= 1e-3 * float(fx["err_rel"])
    if full["name"].startswith("C2"):
        x_ref, its_ref, rr_ref = orc.bicgstab(levels, orc.cycle_opts(smoother=capi.SMOOTH_PATCH_SOLVE), b)
        assert rr_ref <= 1e-12 and rel(x, x_ref) <= 1e-8


# ---------------------------------------------------------------------------------------------- (b)
FIXTURES = sorted(glob.glob(os.path.join(util.GOLDEN, "ref_*_n*.npz")))


@pytest.fixture(scope="module", params=FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def gold(request):
    d = dict(np.load(request.param))
    dim, n, neu = int(d["dim"]), int(d["n"]), bool(int(d["neumann"]))
    m, H, levels = util.setup(str(d["mesh"]), n, 0, neumann=neu, dim=dim)
    g = capi.GMG(H)
    ids = H.tables(0)["id"]
    # golden vectors are in the order of d["t_id"]; this build's order is `ids` (Morton): key by patch id
    pos = {int(i): k for k, i in enumerate(d["t_id"])}
    perm = np.array([pos[int(i)] for i in ids])
    nc = n ** dim

    def mine(v):  # golden order -> this library's order
        return np.ascontiguousarray(v.reshape(-1, nc)[perm]).ravel()

    return dict(d=d, g=g, L=levels[0], mine=mine, dim=dim, n=n, neumann=neu)


def test_hip_apply_equals_reference_apply(gold):
    """te_apply (k_stencil3d / k_stencil2d + coarse/fine ghosts) vs SchurHelper::apply built from the reference's
    compiled TriLinInterp/BilinearInterpolator + StarPatchOp::applyWithInterface (golden `apply`)."""
    d, g, L, mine = gold["d"], gold["g"], gold["L"], gold["mine"]
    du, df = g.new_vector(0, mine(d["u"])), g.new_vector(0)
    g.apply(du, df)
    assert np.abs(df.download() - mine(d["apply"])).max() <= util.op_tol(L, d["u"])


def test_hip_patch_apply_equals_reference_patch_apply(gold):
    """te_patch_apply vs the reference's StarPatchOp::apply (StarPatchOp.h:204-319), golden `patch_apply`."""
    d, g, L, mine = gold["d"], gold["g"], gold["L"], gold["mine"]
    du, df = g.new_vector(0, mine(d["u"])), g.new_vector(0)
    g.patch_apply(du, df)
    assert np.abs(df.download() - mine(d["patch_apply"])).max() <= util.op_tol(L, d["u"])


def test_hip_block_jacobi_sweep_inverts_reference_patch_operator(gold):
    """One block-Jacobi sweep (a8 + a9) u' = S(f, u): the reference's own patch operator applied to u' must give
    the reference's own right-hand side f - (2/h^2) gamma(u) on every patch (SchurHelper.h:318-331,
    FftwPatchSolver.h:173-206 solve exactly that system). Right-hand side: golden `f`, golden `gamma` (= the
    reference's interpolate(u)) through the reference's addInterfaceToRHS when its compiled slice is here, else through
    the oracle's (pinned to golden `add_iface_rhs` by tests/test_oracle_golden.py); operator: te_patch_apply (pinned
    to golden `patch_apply` above) and, when present, the reference's compiled StarPatchOp::apply."""
    d, g, L, mine = gold["d"], gold["g"], gold["L"], gold["mine"]
    if gold["neumann"] and L.P == 1:
        pytest.skip("pure Neumann single patch: singular (tests/test_oracle_golden.py::test_neumann_single_patch)")
    live = refslice.available()
    Lg = orc.Level(gold["dim"], gold["n"], d["t_id"], d["t_h"], d["t_nbr_kind"], d["t_nbr"], d["t_nbr_orth"],
                   d["t_neumann"], d["t_parent"], d["t_orth_on_parent"])  # golden patch order
    rhs = (refslice.add_iface_rhs if live else orc.add_iface_rhs)(Lg, d["gamma"], d["f"])
    du, df, dr = g.new_vector(0, mine(d["u"])), g.new_vector(0, mine(d["f"])), g.new_vector(0)
    g.smooth(df, du, smoother=capi.SMOOTH_PATCH_SOLVE)
    g.patch_apply(du, dr)
    scale = np.abs(rhs).max()
    assert np.abs(dr.download() - mine(rhs)).max() <= 1e-11 * scale
    if live:
        nc = gold["n"] ** gold["dim"]
        ids = gold["g"].hier.tables(0)["id"]
        pos = {int(i): k for k, i in enumerate(d["t_id"])}
        unew = np.empty_like(d["u"])
        unew.reshape(-1, nc)[[pos[int(i)] for i in ids]] = du.download().reshape(-1, nc)  # back to golden order
        assert np.abs(refslice.patch_apply(Lg, unew) - rhs).max() <= 1e-11 * scale


@pytest.mark.parametrize("smoother", [capi.SMOOTH_RBGS, capi.SMOOTH_JACOBI, capi.SMOOTH_PATCH_SOLVE], ids=["rbgs", "jacobi", "patch_solve"])
def test_smoothers_leave_the_reference_operators_solution_alone(gold, smoother):
    """The headline smoother (patch-local RB-GS) and weighted Jacobi have no function in the reference to be compared with sweep by
    sweep; what pins them to the REFERENCE's operator is their defining property: an iterate that already satisfies A u = f is a
    fixed point of the sweep. f := the reference's own compiled SchurHelper::apply of u (golden `apply`: TriLinInterp / Bilinear
    interface values + StarPatchOp::applyWithInterface, coarse/fine faces and Neumann closures included); one sweep from u must
    return u to rounding. A wrong stencil weight, diagonal, ghost or coarse/fine weight in the smoother kernels moves u at O(1).
    (The reference's block-Jacobi sweep, checked against the compiled patch operator above, has the same property.)"""
    d, g, L, mine = gold["d"], gold["g"], gold["L"], gold["mine"]
    if gold["neumann"] and L.P == 1 and smoother == capi.SMOOTH_PATCH_SOLVE:
        pytest.skip("pure Neumann single patch: the exact patch solve is singular")
    u = mine(d["u"])
    du, df = g.new_vector(0, u), g.new_vector(0, mine(d["apply"]))
    g.smooth(df, du, smoother=smoother, omega=0.8)
    got = du.download()
    # one relaxation divides a sum of ~ (4 dim / h^2) |u| by a diagonal of ~ 2 dim / h^2: a few ulps of |u|, times the conditioning
    # of an exact patch solve (~ n^2) for the block-Jacobi sweep
    tol = (1e-13 if smoother != capi.SMOOTH_PATCH_SOLVE else 1e-10) * np.abs(u).max()
    assert np.abs(got - u).max() <= tol, (np.abs(got - u).max(), tol)


def test_hip_bicgstab_equals_reference_bicgstab(gold):
    """unpreconditioned te_bicgstab vs the reference's BiCGStab<D>::solve over its own operator (golden bicg_x/its)."""
    d, g, mine = gold["d"], gold["g"], gold["mine"]
    if "bicg_x" not in d:
        pytest.skip("no solve stored for Neumann fixtures")
    db, dx = g.new_vector(0, mine(d["f"])), g.new_vector(0)
    its, rr = g.bicgstab(dx, db, None)
    want = mine(d["bicg_x"])
    assert rr <= 1e-12
    assert abs(its - int(d["bicg_its"])) <= max(3, int(d["bicg_its"]) // 10)  # rounding-order sensitive
    assert np.linalg.norm(dx.download() - want) <= 1e-9 * np.linalg.norm(want)


def test_hip_vector_ops_equal_reference_vector_ops():
    """every te_vec_* against the reference's Vector<D> virtuals on ValVector<3> (Vector.h:190-321), golden
    ref_vecops.npz (3 patches of 4^3 = 192 values; the device vector is a 512-value level, zero-padded)."""
    z = dict(np.load(os.path.join(util.GOLDEN, "ref_vecops.npz")))
    m, H, levels = util.setup("2uni.bin", 4)
    g = capi.GMG(H)
    size, k = levels[0].size, z["v0"].size
    assert size >= k

    def vec(a):
        p = np.zeros(size)
        p[:k] = a
        return g.new_vector(0, p)

    al, be, ga = float(z["alpha"]), float(z["beta"]), float(z["gamma"])
    ops = {0: lambda v, a, b: v.set(al), 1: lambda v, a, b: v.scale(al), 2: lambda v, a, b: v.shift(al),
           3: lambda v, a, b: v.copy(a), 4: lambda v, a, b: v.add(a), 5: lambda v, a, b: v.addScaled(al, a),
           6: lambda v, a, b: v.addScaled(al, a, be, b), 7: lambda v, a, b: v.scaleThenAdd(al, a),
           8: lambda v, a, b: v.scaleThenAddScaled(al, be, a), 9: lambda v, a, b: v.scaleThenAddScaled(al, be, a, ga, b)}
    for op, fn in ops.items():
        v, a, b = vec(z["v0"]), vec(z["a"]), vec(z["b"])
        fn(v, a, b)
        got = v.download()[:k]
        # one rounding per multiply/add, no reassociation: <= 2 ulp of the largest term (FMA contraction)
        assert np.abs(got - z[f"op{op}"]).max() <= 4 * util.EPS * 8, op
    v, a = vec(z["v0"]), vec(z["a"])
    assert abs(v.dot(a) - z["v0"] @ z["a"]) <= 1e-13 * np.abs(z["v0"]).sum()
    assert abs(v.twoNorm() - np.linalg.norm(z["v0"])) <= 1e-14 * np.linalg.norm(z["v0"])
    assert v.infNorm() == np.abs(z["v0"]).max()


@pytest.mark.skipif(not refslice.available(), reason="oracle/_ref/libte_ref.so (the reference's compiled slice) not shipped")
@pytest.mark.parametrize("name,n,div,dim", [("2refine.bin", 8, 1, 3), ("uniform", 32, 1, 3), ("2refine.bin", 32, 0, 3),
                                            ("2d2ref.bin", 16, 1, 2)])
def test_hip_against_live_reference_code(name, n, div, dim):
    """te_apply and te_patch_apply against the reference's compiled TriLinInterp + StarPatchOp on fresh inputs and at
    patch sizes the golden files do not hold (n = 32: the production kernels)."""
    m, H, levels = util.setup(name, n, div, dim=dim)
    g, L = capi.GMG(H), levels[0]
    u = util.rand_vec(L.size, 91)
    du, df = g.new_vector(0, u), g.new_vector(0)
    g.apply(du, df)
    assert np.abs(df.download() - refslice.apply(L, u)).max() <= util.op_tol(L, u)
    g.patch_apply(du, df)
    assert np.abs(df.download() - refslice.patch_apply(L, u)).max() <= util.op_tol(L, u)
    f = util.rand_vec(L.size, 92) / L.a["h"].min() ** 2
    dff = g.new_vector(0, f)
    g.smooth(dff, du, smoother=capi.SMOOTH_PATCH_SOLVE)
    rhs = refslice.add_iface_rhs(L, refslice.interp(L, u), f)
    assert np.abs(refslice.patch_apply(L, du.download()) - rhs).max() <= 1e-11 * np.abs(rhs).max()


@pytest.mark.parametrize("name,n,div,dim", [("uniform", 8, 1, 3), ("2d2ref.bin", 16, 1, 2)])
def test_patch_operator_leaves_no_trace_on_its_level(name, n, div, dim):
    """te_patch_apply and te_apply_with_interface select the patch operator for their own launch only: te_apply on the same
    level gives the same bits before and after them. (Every patch of these meshes has a neighbour face, the 2D one a
    coarse/fine face as well, so the two operators differ.)"""
    m, H, levels = util.setup(name, n, div, dim=dim)
    g, L = capi.GMG(H), levels[0]
    du = g.new_vector(0, util.rand_vec(L.size, 93))
    d1, d2, d3 = g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.apply(du, d1)
    g.patch_apply(du, d2)
    g.apply(du, d3)
    a1 = d1.download()
    assert np.array_equal(a1, d3.download())
    assert not np.array_equal(a1, d2.download())
    if dim == 3:
        dgamma, d4, d5 = g.new_iface_vector(0), g.new_vector(0), g.new_vector(0)
        g.iface_interp(du, dgamma)
        g.apply_with_interface(du, dgamma, d4)
        g.apply(du, d5)
        assert np.array_equal(a1, d5.download())
