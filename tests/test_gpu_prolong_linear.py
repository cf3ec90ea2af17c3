"""-m gpu: the linear interpolator (TE_INTERP_LINEAR: te_prolong_linear_add, te_gmg_set_interpolator) against its numpy statement
(tests/prolong_util.py; the statement itself is checked on the CPU by tests/test_prolong_host.py) and against a cycle composed
from the oracle's pieces with that statement as its prolongation.

Tolerances. Prolongation: |delta| <= 32 eps * 20 * max|e| -- a corner value of the extended block is at most three face ghosts of
magnitude <= 6 max|e| each (2 gamma - m, coefficient sum 2.5 on a coarse/fine face) minus 2 m, and the three convex combinations
add no growth; a wrong weight or neighbour is off by O(0.1 max|e|). Copy-through patches: bit for bit. Cycle: 1e-10 relative,
the project's cycle tolerance; fuse 1 == 0 and 3 == 2 by checksum. Solve: iterations within +-1 of the CPU composition's (the
project's rule), strictly fewer than DrctIntp's, solutions equal to 1e-8."""
import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi, dist as tedist
from tests import bc_util, prolong_util as pu, util

pytestmark = pytest.mark.gpu

# (mesh, n, divides, dim): uniform levels with one and several blocks per level and the production instantiation (32^3, 8 patches),
# coarse/fine faces and copy-through patches at the smallest and a z-slab patch size, a five-level tree, the 2D kernel
SHAPES = [("uniform", 4, 2, 3), ("uniform", 8, 2, 3), ("uniform", 32, 1, 3), ("2refine.bin", 4, 0, 3), ("2refine.bin", 16, 0, 3),
          ("multi_refine.bin", 8, 0, 3), ("2d2ref.bin", 4, 0, 2), ("2d2ref.bin", 16, 0, 2), ("uniform", 64, 2, 2)]
CASES = [s + (mask,) for s in SHAPES for mask in ((0, 0b111111) + bc_util.MASKS3 if s[3] == 3 else (0, 0b1111) + bc_util.MASKS2)]
FUSED_PROLONG = ("stencil_rbgs_prolong", "rbgs_resweep_prolong", "rbgs_resweep_prolong_fcorr", "fcorr_gather")


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}d-{c[4]:06b}")
def case(request):
    name, n, div, dim, mask = request.param
    orc.set_threads(16)
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    return dict(H=H, levels=levels, g=capi.GMG(H), name=name)


def test_prolong_linear_add_per_level_pair(case):
    """random e, random non-zero u: u is added to; a patch that copies through receives exactly u + e"""
    g, levels = case["g"], case["levels"]
    copies = 0
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        e, u = util.rand_vec(C.size, 60 + l), util.rand_vec(F.size, 80 + l)
        de, du = g.new_vector(l + 1, e), g.new_vector(l, u)
        g.interpolate_linear(de, du, fine_level=l)
        got, want = du.download(), pu.prolong_linear_add(F, C, e, u)
        err, bound = np.abs(got - want).max(), 32 * util.EPS * 20 * np.abs(e).max()
        print(f"level {l}: |delta| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, l
        assert np.array_equal(de.download(), e)
        thru = np.flatnonzero(F.a["orth_on_parent"] < 0)
        copies += len(thru)
        for pf in thru:
            pc = F.a["parent"][pf]
            assert np.array_equal(got.reshape(F.P, -1)[pf], u.reshape(F.P, -1)[pf] + e.reshape(C.P, -1)[pc]), (l, pf)
    if case["name"] != "uniform":
        assert copies > 0


def test_bad_arguments():
    H = capi.Hierarchy(util.mesh("2refine.bin"), 4)
    g, other = capi.GMG(H), capi.GMG(H)
    fine, coarse = g.new_vector(0), g.new_vector(1)
    bad = [lambda: g.interpolate_linear(fine, coarse, fine_level=0),  # swapped
           lambda: g.interpolate_linear(coarse, fine, fine_level=1),
           lambda: g.interpolate_linear(g.new_iface_vector(1), fine, fine_level=0),
           lambda: g.interpolate_linear(coarse, g.new_boundary_vector(0), fine_level=0),
           lambda: g.interpolate_linear(coarse, g.new_face_vector(0), fine_level=0),
           lambda: g.interpolate_linear(other.new_vector(1), fine, fine_level=0),
           lambda: g.interpolate_linear(coarse, fine, fine_level=H.num_levels - 1),
           lambda: g.set_interpolator(2), lambda: g.set_interpolator(-1)]
    for call in bad:
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL
    assert g.interpolator == capi.INTERP_DIRECT
    g.set_interpolator(capi.INTERP_LINEAR)
    assert g.interpolator == capi.INTERP_LINEAR
    g.interpolate_linear(coarse, fine, fine_level=0)


def test_sharded_hierarchy_is_refused_and_direct_still_runs():
    mesh, n = util.mesh("uniform", 2), 8
    fab = tedist.LocalFabric(2)
    hs = [capi.Hierarchy(mesh, n, rank=r, nranks=2) for r in range(2)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)

    def run(r):
        g = gs[r]
        codes = []
        for call in (lambda: g.set_interpolator(capi.INTERP_LINEAR), lambda: g.interpolate_linear(g.new_vector(1), g.new_vector(0), fine_level=0)):
            with pytest.raises(capi.TeError) as e:
                call()
            codes.append((e.value.code, str(e.value)))
        g.set_interpolator(capi.INTERP_DIRECT)
        f, u = g.new_vector(0, util.rand_vec(hs[r].sizes(0)[0] * n ** 3, 5 + r)), g.new_vector(0)
        g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), f, u)
        return codes, g.interpolator, np.isfinite(u.download()).all() and np.abs(u.download()).max() > 0

    for codes, kind, ok in fab.run(run):
        assert [c for c, _ in codes] == [capi.TE_ESTATE, capi.TE_ESTATE], codes
        assert all("sharded" in msg for _, msg in codes), codes
        assert kind == capi.INTERP_DIRECT and ok


SMOOTHERS = [(capi.SMOOTH_RBGS, "rbgs"), (capi.SMOOTH_JACOBI, "jacobi"), (capi.SMOOTH_PATCH_SOLVE, "block_jacobi")]
CYCLES = [((1, 1, 0), "V11"), ((2, 2, 0), "V22"), ((1, 1, 1), "W11")]


@pytest.mark.parametrize("shape", [c[0] for c in CYCLES], ids=[c[1] for c in CYCLES])
@pytest.mark.parametrize("smoother", [s[0] for s in SMOOTHERS], ids=[s[1] for s in SMOOTHERS])
def test_cycle_with_linear_interpolator(case, smoother, shape):
    g, levels = case["g"], case["levels"]
    pre, post, ctype = shape
    f = util.rand_vec(levels[0].size, 70)
    o = g.default_opts(smoother=smoother, pre_sweeps=pre, post_sweeps=post, cycle_type=ctype)
    want = pu.cycle(levels, f, pu.prolong_linear_add, smoother=smoother, pre=pre, post=post, coarse=o.coarse_sweeps, mid=o.mid_sweeps,
                    cycle_type=ctype, omega=o.omega, exact_coarse=o.exact_coarse)
    g.set_interpolator(capi.INTERP_LINEAR)
    sums = {}
    try:
        for fuse in (0, 1, 2, 3):
            o.fuse = fuse
            df, du = g.new_vector(0, f), g.new_vector(0)
            du.set(123.0)  # Cycle::apply ignores the incoming u
            g.cycle(o, df, du)
            err = np.abs(du.download() - want).max() / np.abs(want).max()
            sums[fuse] = du.checksumLocal()
            print(f"fuse={fuse}: relative |delta| = {err:.3e}")
            assert err <= 1e-10, (fuse, err)
    finally:
        g.set_interpolator(capi.INTERP_DIRECT)
    assert sums[1] == sums[0] and sums[3] == sums[2], sums


def profiled_cycle(g, o, f):
    df, du = g.new_vector(0, f), g.new_vector(0)
    g.profile(True)
    g.profile_reset()
    g.cycle(o, df, du)
    rows = g.profile_rows()
    g.profile(False)
    return du.checksumLocal(), {k for k, v in rows.items() if v["calls"] > 0}


@pytest.mark.parametrize("name,n,div,dim", [("uniform", 4, 3, 3), ("2refine.bin", 4, 1, 3), ("uniform", 8, 3, 2)], ids=lambda v: str(v))
def test_default_is_unchanged_and_the_fused_forms_are_off_under_linear(name, n, div, dim):
    """te_vcycle(fuse = 3) gives the same bits on a fresh solver, on one that was set to LINEAR and back, and on one that only
    called te_prolong_linear_add in between; the fused prolongation kernels run under DIRECT and not under LINEAR"""
    H = capi.Hierarchy(util.mesh(name, div, dim), n)
    f = util.rand_vec(H.cells(0), 71)
    for smoother in (capi.SMOOTH_RBGS, capi.SMOOTH_PATCH_SOLVE):
        fresh, toggled, called = capi.GMG(H), capi.GMG(H), capi.GMG(H)
        o = fresh.default_opts(smoother=smoother, fuse=3)
        ref, ran = profiled_cycle(fresh, o, f)
        assert "prolong_linear" not in ran
        if smoother == capi.SMOOTH_RBGS:
            assert ran & set(FUSED_PROLONG), sorted(ran)
        toggled.set_interpolator(capi.INTERP_LINEAR)
        lin, ran_lin = profiled_cycle(toggled, o, f)
        assert "prolong_linear" in ran_lin and not (ran_lin & set(FUSED_PROLONG)) and "prolong_add" not in ran_lin, sorted(ran_lin)
        assert lin != ref
        toggled.set_interpolator(capi.INTERP_DIRECT)
        back, ran_back = profiled_cycle(toggled, o, f)
        assert back == ref and ran_back == ran, (sorted(ran_back), sorted(ran))
        called.interpolate_linear(called.new_vector(1, util.rand_vec(H.cells(1), 72)), called.new_vector(0), fine_level=0)
        assert profiled_cycle(called, o, f) == (ref, ran)


@pytest.mark.parametrize("name,n,div", [("uniform", 8, 2), ("uniform", 4, 2), ("2refine.bin", 8, 0)], ids=lambda v: str(v))
def test_solve_takes_fewer_iterations(name, n, div):
    """V(1,1) with RB-GS, f ~ U(-1, 1) from default_rng(0), to 1e-12: the right-hand side of tests/test_prolong_host.py"""
    orc.set_threads(16)
    m, H, levels = util.setup(name, n, div)
    g = capi.GMG(H)
    f = util.rand_vec(levels[0].size, 0)
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)
    _, cpu_its = pu.bicgstab(levels, f, pu.prolong_linear_add, smoother=capi.SMOOTH_RBGS)
    x_dir, x_lin = g.new_vector(0), g.new_vector(0)
    its_dir, _ = g.bicgstab(x_dir, g.new_vector(0, f), o)
    g.set_interpolator(capi.INTERP_LINEAR)
    its_lin, rr = g.bicgstab(x_lin, g.new_vector(0, f), o)
    print(f"{name} n={n}: iterations linear {its_lin} (CPU composition {cpu_its}), DrctIntp {its_dir}; relative residual {rr:.2e}")
    assert abs(its_lin - cpu_its) <= 1
    assert its_lin < its_dir
    a, b = x_lin.download(), x_dir.download()
    assert np.linalg.norm(a - b) <= 1e-8 * np.linalg.norm(b)
