"""GPU: the Schur-complement route (te_iface_interp ... te_schur_solve) against the reference's compiled interface primitives
(tests/golden/ref_*.npz), the CPU oracle's composition of the same operators, and -- the headline property -- the domain solve:
u from S gamma = g followed by u = Solve(f, gamma) is u from te_bicgstab with the GMG cycle."""
import glob
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import refslice
from pressurepoissonsolver_amd import capi, solver
from tests import util

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(util.GOLDEN, "ref_*_n*.npz")))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def level_of(d):
    return orc.Level(int(d["dim"]), int(d["n"]), d["t_id"], d["t_h"], d["t_nbr_kind"], d["t_nbr"], d["t_nbr_orth"], d["t_neumann"],
                     d["t_parent"], d["t_orth_on_parent"])


@pytest.fixture(scope="module", params=FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def gold(request):
    orc.set_threads(16)
    d = dict(np.load(request.param))
    H = capi.Hierarchy(util.mesh(str(d["mesh"]), 0, int(d["dim"])), int(d["n"]), neumann=bool(d["neumann"]))
    return d, level_of(d), capi.GMG(H)


def cpu_T(L, x):
    return orc.interp(L, orc.patch_solve(L, x, np.zeros(L.size)))


def test_interp_apply_and_rhs_equal_reference_goldens(gold):
    d, L, g = gold
    du, dg, df = g.new_vector(0, d["u"]), g.new_iface_vector(0), g.new_vector(0)
    g.iface_interp(du, dg)
    if L.num_ifaces():
        assert np.abs(dg.download() - d["gamma"]).max() <= 4 * util.EPS * np.abs(d["u"]).max()
    dgi = g.new_iface_vector(0, d["gamma_in"])
    g.apply_with_interface(du, dgi, df)
    tol = util.op_tol(L, np.concatenate([d["u"], d["gamma_in"]]))
    assert np.abs(df.download() - d["apply_with_gamma"]).max() <= tol
    df.upload(d["f"])
    g.add_iface_rhs(dgi, df)
    assert np.abs(df.download() - d["add_iface_rhs"]).max() <= util.op_tol(L, np.concatenate([d["f"] * L.a["h"].min() ** 2, d["gamma_in"]]))


def test_solve_and_schur_apply_equal_cpu_composition(gold):
    d, L, g = gold
    nif = L.num_ifaces()
    x = util.rand_vec(nif * L.nf, 5)
    f = util.rand_vec(L.size, 6) / L.a["h"].min() ** 2
    dx, dy, du, dd = g.new_iface_vector(0, x), g.new_iface_vector(0), g.new_vector(0), g.new_iface_vector(0)
    g.solve_with_interface(g.new_vector(0, f), du, dx, dd)
    want = orc.patch_solve(L, x, f)
    assert rel(du.download(), want) <= 1e-12
    if nif:
        assert rel(dd.download(), orc.interp(L, want) - x) <= 1e-12
        g.schur_apply(dx, dy)
        assert rel(dy.download(), x - cpu_T(L, x)) <= 1e-12


def test_live_slice_interp_n32():
    if not refslice.available():
        pytest.skip("reference slice not built")
    m, H, levels = util.setup("2refine.bin", 32)
    g, L = capi.GMG(H), levels[0]
    u = util.rand_vec(L.size, 9)
    dg = g.new_iface_vector(0)
    g.iface_interp(g.new_vector(0, u), dg)
    assert np.abs(dg.download() - refslice.interp(L, u)).max() <= 4 * util.EPS * np.abs(u).max()


@pytest.mark.parametrize("mode", ["1pass", "3pass"])
@pytest.mark.parametrize("name", ["2uni.bin", "2refine.bin"])
def test_schur_apply_both_32_cube_paths(name, mode):
    orc.set_threads(16)
    m, H, levels = util.setup(name, 32)
    g, L = capi.GMG(H), levels[0]
    g.set_option("TE_PS_MODE", mode)
    x = util.rand_vec(H.num_ifaces(0) * L.nf, 11)
    dy = g.new_iface_vector(0)
    g.schur_apply(g.new_iface_vector(0, x), dy)
    assert rel(dy.download(), x - cpu_T(L, x)) <= 1e-12
    f = util.rand_vec(L.size, 12)
    du = g.new_vector(0)
    g.solve_with_interface(g.new_vector(0, f), du, g.new_iface_vector(0, x))
    assert rel(du.download(), orc.patch_solve(L, x, f)) <= 1e-12


def test_schur_apply_2d_64():
    orc.set_threads(16)
    m, H, levels = util.setup("2d2ref.bin", 64, dim=2)
    g, L = capi.GMG(H), levels[0]
    x = util.rand_vec(H.num_ifaces(0) * L.nf, 13)
    dy = g.new_iface_vector(0)
    g.schur_apply(g.new_iface_vector(0, x), dy)
    assert rel(dy.download(), x - cpu_T(L, x)) <= 1e-12


def test_faces_only_apply_is_bit_identical_to_full():
    """256^3 in 32^3 patches: T takes k_ps_sym<CORR, FACES, NOF> (six face layers out) by default, the full solve under TE_SCHUR_FULL"""
    H = capi.Hierarchy(capi.Mesh.uniform(3, 3), 32)
    g = capi.GMG(H)
    x = util.rand_vec(H.num_ifaces(0) * 32 * 32, 17)
    dx, got = g.new_iface_vector(0, x), {}
    for full in (None, "1"):
        g.set_option("TE_SCHUR_FULL", full)
        g.profile(True)
        g.profile_reset()
        dy = g.new_iface_vector(0)
        g.schur_apply(dx, dy)
        rows = g.profile_rows()
        g.profile(False)
        got[full] = dy.download()
        assert ("patch_solve_mfma_faces" in rows) == (full is None)
    assert np.array_equal(got[None], got["1"])


def cheb_coeffs():
    a, b = 1 - 0.475, 0.475
    s = np.sqrt(a * a - b * b)
    r = (a - s) / b
    return np.array([1 / s] + [2 * r ** k / s for k in range(1, 16)])


def test_cheb_equals_numpy_clenshaw():
    orc.set_threads(16)
    m, H, levels = util.setup("2refine.bin", 8)
    g, L = capi.GMG(H), levels[0]
    x = util.rand_vec(H.num_ifaces(0) * L.nf, 19)
    c = cheb_coeffs()
    b1, b2 = np.zeros_like(x), np.zeros_like(x)
    for i in range(15, 0, -1):
        b = 4 / 0.95 * cpu_T(L, b1) - 2 * b1 + c[i] * x - b2
        b2, b1 = b1, b
    want = 2 / 0.95 * cpu_T(L, b1) - b1 + c[0] * x - b2
    dy = g.new_iface_vector(0)
    g.schur_cheb(g.new_iface_vector(0, x), dy)
    assert rel(dy.download(), want) <= 1e-11


def domain_solve(g, df, check=True):
    du = g.new_vector(0)
    its, rr = g.bicgstab(du, df, g.default_opts(), tol=1e-12)
    assert rr <= 1e-12 or not check
    return du.download()


@pytest.mark.parametrize("name,div,n,dim", [("uniform", 3, 32, 3), ("2refine.bin", 1, 32, 3), ("2d2ref.bin", 0, 64, 2)],
                         ids=["256cube-32", "2refine-div1-32", "2d2ref-64"])
def test_schur_solve_equals_domain_solve(name, div, n, dim):
    H = capi.Hierarchy(util.mesh(name, div, dim), n)
    g = capi.GMG(H)
    df = g.new_vector(0)
    g.init_problem(df, problem=capi.PROBLEM_TRIG)
    want = domain_solve(g, df)
    for prec in (None, "cheb"):
        du = g.new_vector(0)
        its, rr, gamma = solver.schur_solve(g, df, du, prec=prec, tol=1e-12)
        assert its > 0 and rr <= 1e-12, (prec, its, rr)
        assert np.abs(du.download() - want).max() <= 1e-8 * np.abs(want).max(), prec
        diff = g.new_iface_vector(0)
        dg = g.new_iface_vector(0)
        g.solve_with_interface(df, du, gamma, diff)
        # |g| with g = Interp(Solve(f, 0))
        g.iface_interp(_solve0(g, H, df), dg)
        assert diff.twoNorm() <= 1e-10 * dg.twoNorm()


def _solve0(g, H, df):
    du = g.new_vector(0)
    g.solve_with_interface(df, du, g.new_iface_vector(0))
    return du


def test_schur_solve_neumann():
    H = capi.Hierarchy(util.mesh("2refine.bin", 0, 3), 16, neumann=True)
    g = capi.GMG(H)
    df = g.new_vector(0)
    g.init_problem(df, problem=capi.PROBLEM_TRIG, neumann=True)
    df.shift(-g.integrate(df) / g.volume())  # apps/3d/steady.cpp:330-334
    want = domain_solve(g, df)
    want -= want.mean()
    dg = g.new_iface_vector(0)
    g.iface_interp(_solve0(g, H, df), dg)
    for prec in (None, "cheb"):
        du = g.new_vector(0)
        its, rr, gamma = solver.schur_solve(g, df, du, prec=prec, tol=1e-12)
        assert its > 0 and rr <= 1e-12, (prec, its, rr)
        got = du.download()
        got -= got.mean()
        assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), (prec, its, rr)
        diff = g.new_iface_vector(0)
        g.solve_with_interface(df, du, gamma, diff)
        assert diff.twoNorm() <= 1e-10 * dg.twoNorm(), prec


def test_single_patch_takes_no_iteration():
    orc.set_threads(16)
    m, H, levels = util.setup("1uni.bin", 8)
    g, L = capi.GMG(H), levels[0]
    assert H.num_ifaces(0) == 0
    f = util.rand_vec(L.size, 23)
    du = g.new_vector(0)
    its, rr, gamma = solver.schur_solve(g, g.new_vector(0, f), du, prec="cheb")
    assert its == 0 and gamma.size == 0
    assert rel(du.download(), orc.patch_solve(L, np.zeros(0), f)) <= 1e-12


def test_interface_vector_is_refused_by_domain_operators():
    H = capi.Hierarchy(util.mesh("2uni.bin"), 8)
    g = capi.GMG(H)
    gi, du = g.new_iface_vector(0), g.new_vector(0)
    for call in (lambda: g.apply(gi, du), lambda: g.apply(du, gi), lambda: g.cycle(g.default_opts(), gi, du),
                 lambda: g.smooth(gi, du)):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL
    with pytest.raises(capi.TeError) as e:
        du.copy(gi)
    assert e.value.code == capi.TE_EINVAL
    # aliased arguments of the Schur entry points
    gj = g.new_iface_vector(0)
    for call in (lambda: g.solve_with_interface(du, g.new_vector(0), gi, gi), lambda: g.schur_apply(gi, gi),
                 lambda: g.schur_cheb(gi, gi), lambda: g.solve_with_interface(du, du, gi, gj)):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL


def test_sharded_hierarchy_is_refused():
    H = capi.Hierarchy(util.mesh("2uni.bin"), 8, rank=0, nranks=2)
    g = capi.GMG(H)
    with pytest.raises(capi.TeError) as e:
        g.new_iface_vector(0)
    assert e.value.code == capi.TE_ESTATE
    du, dv = g.new_vector(0), g.new_vector(0)
    with pytest.raises(capi.TeError) as e:
        g.iface_interp(du, dv)
    assert e.value.code == capi.TE_ESTATE
