"""-m gpu: te_cell_slopes, te_advect_flux_muscl and te_advect_muscl (include/te_hip.h) against the numpy
statement of tests/muscl_util.py, which tests/test_muscl_host.py checks on its own.

Shapes, masks, inputs and helpers are tests/test_gpu_advect.py's: every level of each, with a boundary vector and without, for
MINMOD, MC and CENTRAL. One statement per (shape, mask, level, cb, kind), computed once and shared.

Bounds (none of them comes from what the kernels give):
  cell_slopes, advect_flux_muscl   bit for bit: every operation of the rules is rounded on its own, the means in a fixed order
  fused = composed                 te_advect_muscl against te_advect_flux_muscl, te_divergence, te_vec_copy, te_vec_add_scaled: bit for bit
  ZERO                             te_advect_flux's and te_advect's values
  slab counts                      every ZS > 1 output of the two marches and of the slope pass equals the ZS = 1 output bit for bit
  conservation, positivity         tests/test_muscl_host.py's statements, on the device's own output
  order                            test_muscl_host's five gates on the device's own run; the final field within 1e-12 of the
                                   statement's: 128 calls of at most a dozen roundings of O(1) values, about 2e-13 (the limiters are
                                   continuous, so a flipped branch moves S by rounding only)"""
import functools
import math

import numpy as np
import pytest

from pressurepoissonsolver_amd import capi, dist as tedist
from tests import advect_util as au, bc_util, muscl_util as mu, projection_util as pu, util
from tests import test_muscl_host as host
from tests.test_gpu_advect import ALPHA, CASES, IDS, SLABS, inputs, pinned, solver

pytestmark = pytest.mark.gpu

EPS = util.EPS
KINDS = (mu.MINMOD, mu.MC, mu.CENTRAL)


@functools.lru_cache(maxsize=None)
def statement(key, l, with_cb, kind):
    """(the slopes as one array [dim * size], the packed flux) of the statement"""
    S, d = solver(*key), inputs(key, l)
    L, cb = S.levels[l], (d.cb if with_cb else None)
    return (mu.cell_slopes(L, d.c, kind, cb).reshape(S.dim, -1), pu.pack(*mu.advect_flux(L, pu.unpack(d.U, S.n, S.dim), d.c, kind, cb)))


def run(S, l, with_cb, kind):
    """the device's slopes, flux, fused update and composed update of level l"""
    g, d, dim = S.g, inputs(S.key, l), S.dim
    dU, dc, dcb = g.new_face_vector(l, d.U), g.new_vector(l, d.c), g.new_boundary_vector(l, d.cb if d.cb.size else None)
    b = dcb if with_cb else None
    dS = [g.new_vector(l) for _ in range(dim)]
    dF, out, comp, dd = g.new_face_vector(l), g.new_vector(l), g.new_vector(l), g.new_vector(l)
    for v in dS + [dF, out]:
        v.set(-7.0)
    g.cell_slopes(dc, dS[0], dS[1], dS[2] if dim == 3 else None, kind=kind, cb=b, level=l)
    g.advect_flux_muscl(dU, dc, dF, kind=kind, cb=b, level=l)
    g.advect_muscl(dU, dc, out, alpha=ALPHA, kind=kind, cb=b, level=l)
    g.divergence(dF, dd, alpha=ALPHA, level=l)
    comp.copy(dc)
    comp.addScaled(-1.0, dd)
    return np.stack([v.download() for v in dS]), dF.download(), out.download(), comp.download()


@pytest.mark.parametrize("name,div,mask,n,dim", CASES, ids=IDS)
def test_against_the_statement_and_fused_equals_composed(name, div, mask, n, dim):
    S = solver(name, div, mask, n, dim)
    g = S.g
    assert len(S.levels) >= 2
    for l, L in enumerate(S.levels):
        d = inputs(S.key, l)
        for with_cb in (False, True):
            for kind in KINDS:
                slopes, F, fused, comp = run(S, l, with_cb, kind)
                want_s, want_f = statement(S.key, l, with_cb, kind)
                print(f"level {l} cb={with_cb} kind {kind}: slopes differ in {int((slopes != want_s).sum())} entries, the flux in "
                      f"{int((F != want_f).sum())}, fused from composed in {int((fused != comp).sum())} cells")
                assert np.array_equal(slopes, want_s), (l, with_cb, kind, np.abs(slopes - want_s).max())
                assert np.array_equal(F, want_f), (l, with_cb, kind, np.abs(F - want_f).max())
                assert np.array_equal(fused, comp), (l, with_cb, kind, np.abs(fused - comp).max(), int((fused != comp).sum()))
                assert not np.array_equal(fused, d.c)
                dF = g.new_face_vector(l, F)  # the flux is a fixed point of the matching
                g.faces_match(dF, level=l)
                assert np.array_equal(dF.download(), F), (l, with_cb, kind)
            # ZERO: te_advect_flux's and te_advect's values
            slopes, F, fused, _ = run(S, l, with_cb, mu.ZERO)
            dU, dc = g.new_face_vector(l, d.U), g.new_vector(l, d.c)
            b = g.new_boundary_vector(l, d.cb if d.cb.size else None) if with_cb else None
            dF, out = g.new_face_vector(l), g.new_vector(l)
            g.advect_flux(dU, dc, dF, cb=b, level=l)
            g.advect(dU, dc, out, alpha=ALPHA, cb=b, level=l)
            assert not slopes.any()
            assert np.array_equal(F, dF.download()) and np.array_equal(fused, out.download()), (l, with_cb)
            assert not np.array_equal(F, statement(S.key, l, with_cb, mu.MC)[1])


@functools.lru_cache(maxsize=None)
def slab_run(key, zs):
    S = solver(*key)
    out = {}
    with pinned(S.g, zs):
        for l in range(len(S.levels)):
            out[l, "slopes"], out[l, "flux"], out[l, "fused"], _ = run(S, l, True, mu.MC)
    return out


@pytest.mark.parametrize("name,n,zs", SLABS, ids=[f"{c[0]}-n{c[1]}-zs{c[2]}" for c in SLABS])
def test_every_slab_instantiation_gives_the_bits_of_one_slab(name, n, zs):
    S = solver(name, 1 if name == "uniform" else 0, bc_util.CHANNEL, n, 3)
    base = slab_run(S.key, 1)
    got = slab_run(S.key, zs)
    for k in base:
        assert np.array_equal(got[k], base[k]), k


@pytest.mark.parametrize("key", [("2refine.bin", 0, 0, 4, 3), ("uniform", 1, 0, 32, 3), ("2d2ref.bin", 0, 0, 8, 2)], ids=lambda k: f"{k[0]}-n{k[3]}-{k[4]}d")
def test_conservation_and_positivity_on_the_device(key):
    S = solver(*key)
    g, n, dim = S.g, S.n, S.dim
    for l, L in enumerate(S.levels):
        d = inputs(S.key, l)
        c = np.where(np.random.default_rng(7).random(d.c.size) < 0.2, 0.0, d.c)
        dc, dcb, out, dF = g.new_vector(l, c), g.new_boundary_vector(l, d.cb if d.cb.size else None), g.new_vector(l), g.new_face_vector(l)
        # conservation: U = 0 on the physical faces; the bound from the device's own flux
        U0 = pu.pack(*au.single_valued(L, pu.unpack(d.U, n, dim), zero_physical=True))
        dU = g.new_face_vector(l, U0)
        alpha = 0.9 / (dim * g.faces_max_rate(dU, level=l))
        for kind in (mu.MINMOD, mu.MC):
            g.advect_flux_muscl(dU, dc, dF, kind=kind, level=l)
            g.advect_muscl(dU, dc, out, alpha=alpha, kind=kind, level=l)
            total = abs(math.fsum(((out.download() - c) * au.cell_volumes(L)).tolist()))
            bound = 16 * EPS * alpha * au.flux_area_sum(L, pu.unpack(dF.download(), n, dim))
            print(f"level {l} kind {kind}: imbalance {total:.3e}, {total / bound:.3f} of the bound")
            assert total <= bound, (l, kind, total, bound)
        # positivity: alpha K dim rate = 1 for any velocity (tests/test_muscl_host.py)
        dU.upload(d.U)
        a = 1.0 / (mu.positivity_factor(L) * dim * g.faces_max_rate(dU, level=l))
        for b in (None, dcb):
            for kind in mu.LIMITED:
                g.advect_muscl(dU, dc, out, alpha=a, kind=kind, cb=b, level=l)
                assert out.download().min() >= 0.0, (l, kind)


def test_the_worst_coarse_cell_on_the_device():
    """test_muscl_host's cell beside a coarse/fine face: negative with alpha 2 dim rate = 1 under MC, not with 2.5"""
    S = solver("2d2ref.bin", 0, 0, 8, 2)
    g, L = S.g, S.levels[0]
    c, U, at = host.worst_coarse_cell(L)
    dU, dc, out = g.new_face_vector(0, pu.pack(*U)), g.new_vector(0, c), g.new_vector(0)
    rate = g.faces_max_rate(dU)
    assert rate == 1.0
    g.advect_muscl(dU, dc, out, alpha=1.0 / (2 * 2 * rate), kind=mu.MC)
    assert out.download()[at] == 1.0 - 4.5 / 4
    g.advect_muscl(dU, dc, out, alpha=1.0 / (2.5 * 2 * rate), kind=mu.MC)
    assert out.download().min() >= 0.0


@functools.lru_cache(maxsize=None)
def device_run(cells, kind):
    H, L, c0, exact, alpha, steps = host.order_problem(cells)
    g = capi.GMG(H)
    dU, c, c1, c2 = g.new_face_vector(0, pu.pack(*host.constant_velocity(L))), g.new_vector(0, c0), g.new_vector(0), g.new_vector(0)
    for _ in range(steps):  # Heun: c <- 0.5 (c + adv(adv(c)))
        g.advect_muscl(dU, c, c1, alpha=alpha, kind=kind)
        g.advect_muscl(dU, c1, c2, alpha=alpha, kind=kind)
        c.add(c2)
        c.scale(0.5)
    got = c.download()
    return got, float(np.abs(got - exact).mean())


def test_order_of_accuracy_on_the_device():
    err = {}
    for kind in (mu.ZERO, mu.MC, mu.CENTRAL):
        err[kind] = {}
        for cells in (32, 64):
            got, err[kind][cells] = device_run(cells, kind)
            want = host.statement_run(cells, kind)[0]
            print(f"kind {kind} {cells}^2: the device's field differs from the statement's by {np.abs(got - want).max():.3e}")
            assert np.abs(got - want).max() <= 1e-12, (kind, cells)
    host.order_gates(err)


def test_profile_rows_name_the_three_classes():
    S = solver("2refine.bin", 0, 0, 4, 3)
    g, d = S.g, inputs(S.key, 0)
    dU, dF, dc = g.new_face_vector(0, d.U), g.new_face_vector(0), g.new_vector(0, d.c)
    g.profile(True)
    g.profile_reset()
    g.cell_slopes(dc, g.new_vector(0), g.new_vector(0), g.new_vector(0))
    g.advect_flux_muscl(dU, dc, dF)
    g.advect_muscl(dU, dc, g.new_vector(0))
    rows = g.profile_rows()
    g.profile(False)
    assert rows["cell_slopes"]["calls"] == 3 and rows["cell_slopes"]["cells"] == 3 * S.H.cells(0), sorted(rows)
    for k in ("advect_flux_muscl", "advect_muscl"):
        assert k in rows and rows[k]["calls"] == 1 and rows[k]["cells"] == S.H.cells(0), (k, sorted(rows))
    assert rows["cf_ghost"]["calls"] == 5  # the raw slots once per slope pass, the flux slots once per march


@pytest.mark.parametrize("key", [("2refine.bin", 0, bc_util.CHANNEL, 8, 3), ("2d2ref.bin", 0, bc_util.MASKS2[0], 8, 2)], ids=["3d", "2d"])
def test_the_calls_leave_the_solver_as_it_was(key):
    S = solver(*key)
    g, dim = S.g, S.dim
    f = g.new_vector(0, util.rand_vec(S.levels[0].size, 3))
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)  # V(1,1)

    def cycle_bits():
        u = g.new_vector(0)
        g.cycle(o, f, u)
        return u.download()

    before = cycle_bits()
    for l in range(g.num_levels):
        d = inputs(S.key, l)
        dU, dF, dc = g.new_face_vector(l, d.U), g.new_face_vector(l), g.new_vector(l, d.c)
        g.cell_slopes(dc, g.new_vector(l), g.new_vector(l), g.new_vector(l) if dim == 3 else None, cb=g.new_boundary_vector(l, d.cb), level=l)
        g.advect_flux_muscl(dU, dc, dF, cb=g.new_boundary_vector(l, d.cb), level=l)
        g.advect_muscl(dU, dc, g.new_vector(l), alpha=0.5, kind=mu.MINMOD, level=l)
    assert not g.has_coefficient() and not g.has_reaction()
    assert np.array_equal(cycle_bits(), before)
    # the flux slots right in front of an operator application: te_apply refills the ghost slots it reads
    d = inputs(S.key, 0)
    u, A0, A1, out = g.new_vector(0, d.c), g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.apply(u, A0)
    dU = g.new_face_vector(0, d.U)
    g.advect_muscl(dU, u, out)
    first = out.download()
    g.apply(u, A1)
    assert np.array_equal(A0.download(), A1.download())
    # the solver's slope vectors go with the workspace and come back at the next call
    capi.check(capi.lib().te_gmg_release_workspace(g.h))
    g.advect_muscl(dU, u, out)
    assert np.array_equal(out.download(), first)
    assert np.array_equal(cycle_bits(), before)


def test_refusals():
    S, S2, S2d = solver("2refine.bin", 0, bc_util.CHANNEL, 4, 3), solver("uniform", 2, bc_util.CHANNEL, 4, 3), solver("2d2ref.bin", 0, 0, 8, 2)
    g, g2, gd = S.g, S2.g, S2d.g
    c, c2, c3, c4, c1, U, F, F1, b, b1, i = (g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(1), g.new_face_vector(0),
                                             g.new_face_vector(0), g.new_face_vector(1), g.new_boundary_vector(0), g.new_boundary_vector(1),
                                             g.new_iface_vector(0))
    oc, oF, ob = g2.new_vector(0), g2.new_face_vector(0), g2.new_boundary_vector(0)
    e, e2, e3, e4 = gd.new_vector(0), gd.new_vector(0), gd.new_vector(0), gd.new_vector(0)
    lib, NULL = capi.lib(), None
    MC = capi.SLOPE_MC
    einval = [
        # te_cell_slopes: NULL, aliasing, wrong kind of vector, level, solver, kind; sz in 2D and 3D
        lambda: capi.check(lib.te_cell_slopes(NULL, 0, MC, c.h, NULL, c2.h, c3.h, c4.h)), lambda: capi.check(lib.te_cell_slopes(g.h, 0, MC, NULL, NULL, c2.h, c3.h, c4.h)),
        lambda: capi.check(lib.te_cell_slopes(g.h, 0, MC, c.h, NULL, NULL, c3.h, c4.h)), lambda: capi.check(lib.te_cell_slopes(g.h, 0, MC, c.h, NULL, c2.h, NULL, c4.h)),
        lambda: g.cell_slopes(c, c2, c3, None), lambda: gd.cell_slopes(e, e2, e3, e4),
        lambda: g.cell_slopes(c, c, c3, c4), lambda: g.cell_slopes(c, c2, c, c4), lambda: g.cell_slopes(c, c2, c3, c), lambda: g.cell_slopes(c, c2, c2, c4),
        lambda: g.cell_slopes(c, c2, c3, c3), lambda: g.cell_slopes(c, c2, c3, c2), lambda: gd.cell_slopes(e, e2, e2), lambda: gd.cell_slopes(e, e, e2),
        lambda: g.cell_slopes(F, c2, c3, c4), lambda: g.cell_slopes(c, F, c3, c4), lambda: g.cell_slopes(c, c2, b, c4), lambda: g.cell_slopes(c, c2, c3, i),
        lambda: g.cell_slopes(c, c2, c3, c4, cb=c), lambda: g.cell_slopes(c, c2, c3, c4, cb=b1), lambda: g.cell_slopes(c1, c2, c3, c4),
        lambda: g.cell_slopes(c, c1, c3, c4), lambda: g.cell_slopes(c, c2, c3, c4, level=1), lambda: g.cell_slopes(c, c2, c3, c4, level=-1),
        lambda: g.cell_slopes(c, c2, c3, c4, level=g.num_levels), lambda: g.cell_slopes(oc, c2, c3, c4), lambda: g.cell_slopes(c, c2, c3, oc),
        lambda: g.cell_slopes(c, c2, c3, c4, cb=ob), lambda: g.cell_slopes(c, c2, c3, c4, kind=-1), lambda: g.cell_slopes(c, c2, c3, c4, kind=4),
        # te_advect_flux_muscl
        lambda: capi.check(lib.te_advect_flux_muscl(g.h, 0, MC, NULL, c.h, NULL, F.h)), lambda: capi.check(lib.te_advect_flux_muscl(g.h, 0, MC, U.h, NULL, NULL, F.h)),
        lambda: capi.check(lib.te_advect_flux_muscl(g.h, 0, MC, U.h, c.h, NULL, NULL)), lambda: capi.check(lib.te_advect_flux_muscl(NULL, 0, MC, U.h, c.h, NULL, F.h)),
        lambda: g.advect_flux_muscl(U, c, U), lambda: g.advect_flux_muscl(c, c, F), lambda: g.advect_flux_muscl(U, F, F), lambda: g.advect_flux_muscl(U, c, c),
        lambda: g.advect_flux_muscl(U, b, F), lambda: g.advect_flux_muscl(U, i, F), lambda: g.advect_flux_muscl(U, c, F, cb=c), lambda: g.advect_flux_muscl(U, c, F, cb=i),
        lambda: g.advect_flux_muscl(F1, c, F), lambda: g.advect_flux_muscl(U, c1, F), lambda: g.advect_flux_muscl(U, c, F1), lambda: g.advect_flux_muscl(U, c, F, cb=b1),
        lambda: g.advect_flux_muscl(U, c, F, level=1), lambda: g.advect_flux_muscl(U, c, F, level=-1), lambda: g.advect_flux_muscl(U, c, F, level=g.num_levels),
        lambda: g.advect_flux_muscl(oF, c, F), lambda: g.advect_flux_muscl(U, oc, F), lambda: g.advect_flux_muscl(U, c, oF), lambda: g.advect_flux_muscl(U, c, F, cb=ob),
        lambda: g.advect_flux_muscl(U, c, F, kind=-1), lambda: g.advect_flux_muscl(U, c, F, kind=4),
        # te_advect_muscl
        lambda: capi.check(lib.te_advect_muscl(g.h, 0, 1.0, MC, NULL, c.h, NULL, c2.h)), lambda: capi.check(lib.te_advect_muscl(g.h, 0, 1.0, MC, U.h, NULL, NULL, c2.h)),
        lambda: capi.check(lib.te_advect_muscl(g.h, 0, 1.0, MC, U.h, c.h, NULL, NULL)), lambda: capi.check(lib.te_advect_muscl(NULL, 0, 1.0, MC, U.h, c.h, NULL, c2.h)),
        lambda: g.advect_muscl(U, c, c), lambda: g.advect_muscl(c, c, c2), lambda: g.advect_muscl(U, F, c2), lambda: g.advect_muscl(U, c, F), lambda: g.advect_muscl(U, c, b),
        lambda: g.advect_muscl(U, c, c2, cb=F), lambda: g.advect_muscl(F1, c, c2), lambda: g.advect_muscl(U, c1, c2), lambda: g.advect_muscl(U, c, c1),
        lambda: g.advect_muscl(U, c, c2, cb=b1), lambda: g.advect_muscl(U, c, c2, level=1), lambda: g.advect_muscl(oF, c, c2), lambda: g.advect_muscl(U, oc, c2),
        lambda: g.advect_muscl(U, c, oc), lambda: g.advect_muscl(U, c, c2, cb=ob), lambda: g.advect_muscl(U, c, c2, kind=-1), lambda: g.advect_muscl(U, c, c2, kind=4),
    ]
    for k, call in enumerate(einval):
        with pytest.raises(capi.TeError) as err:
            call()
        assert err.value.code == capi.TE_EINVAL, k
    for kind in mu.KINDS:  # ... and every kind there is goes through
        g.advect_muscl(U, c, c2, kind=kind)


def test_a_sharded_hierarchy_is_refused_and_still_cycles():
    """two virtual ranks with a fabric attached: the three calls answer TE_ESTATE ("sharded"), a DIRECT cycle runs afterwards"""
    mesh = util.mesh("uniform", 2, 3)
    fab = tedist.LocalFabric(2)
    fab.timeout = 30.0
    hs = [capi.Hierarchy(mesh, 8, rank=r, nranks=2) for r in range(2)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)

    def per_rank(r):
        g = gs[r]
        c, out, U, F = g.new_vector(0), g.new_vector(0), g.new_face_vector(0), g.new_face_vector(0)
        seen = []
        for call in (lambda: g.cell_slopes(c, out, g.new_vector(0), g.new_vector(0)), lambda: g.advect_flux_muscl(U, c, F), lambda: g.advect_muscl(U, c, out)):
            with pytest.raises(capi.TeError) as e:
                call()
            seen.append((e.value.code, "sharded" in str(e.value)))
        assert g.interpolator == capi.INTERP_DIRECT
        f, u = g.new_vector(0), g.new_vector(0)
        f.set(1.0)
        g.cycle(g.default_opts(smoother=capi.SMOOTH_RBGS), f, u)
        return seen, u.infNorm() if u.size else 0.0

    outs = fab.run(per_rank)
    for seen, norm in outs:
        assert seen == [(capi.TE_ESTATE, True)] * 3, seen
    assert max(norm for _, norm in outs) > 0.0
