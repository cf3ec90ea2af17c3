"""-m gpu: te_advect_flux, te_advect, te_faces_match and te_faces_max_rate (include/te_hip.h) against the numpy
statement of tests/advect_util.py, which tests/test_advect_host.py checks on its own.

Shapes: the smallest at which each code path exists -- 4^3 patches (one slab only), 8^3, 32^3 (slabs), 2refine.bin at 4^3 and 16^3
(coarse/fine faces, copy-through patches), 2D uniform and 2d2ref.bin at 8^2 -- every level of each, all-Dirichlet and under one mixed
mask, with a boundary vector and without. U is random with both signs and some exact zeros. One statement per (shape, mask, level),
computed once and shared.

Bounds (none of them comes from what the kernels give):
  advect_flux, faces_match, faces_max_rate   bit for bit: one product per entry, the means in a fixed order, one correctly rounded
                                             division per entry and a maximum
  fused = composed                           te_advect against te_advect_flux, te_divergence, te_vec_copy, te_vec_add_scaled: bit for bit
  slab counts                                every ZS > 1 output of k_advect3d / k_advflux3d equals the ZS = 1 output bit for bit
  conservation, positivity                   tests/test_advect_host.py's statements, on the device's own output"""
import contextlib
import functools
import math
import types

import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi, dist as tedist
from tests import advect_util as au, bc_util, projection_util as pu, util

pytestmark = pytest.mark.gpu

EPS = util.EPS
PIN = "TE_ZS_PIN"
SHAPES = [("uniform", 2, 4, 3), ("uniform", 2, 8, 3), ("uniform", 1, 32, 3), ("2refine.bin", 0, 4, 3), ("2refine.bin", 0, 16, 3),
          ("uniform", 3, 8, 2), ("2d2ref.bin", 0, 8, 2)]
CASES = [(name, div, mask, n, dim) for name, div, n, dim in SHAPES for mask in (0, bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0])]
IDS = [f"{c[0]}-{c[2]:06b}-n{c[3]}-{c[4]}d" for c in CASES]
SLABS = [(name, n, zs) for name in ("uniform", "2refine.bin") for n, counts in ((16, (2, 4)), (32, (2, 4, 8))) for zs in counts]
ALPHA = 0.37


@functools.lru_cache(maxsize=None)
def solver(name, div, mask, n, dim):
    """one hierarchy and one solver per (mesh, mask, patch size)"""
    orc.set_threads(16)
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    return types.SimpleNamespace(H=H, levels=levels, g=capi.GMG(H), n=n, dim=dim, key=(name, div, mask, n, dim))


@contextlib.contextmanager
def pinned(g, zs):
    try:
        g.set_option(PIN, zs)
        for l in range(g.num_levels):  # the rule returns `zs` on every level about to be used -- asked of the solver, not assumed
            assert g.slab_count(l, capi.SLABS_STENCIL) == zs, (l, zs)
        yield
    finally:
        g.set_option(PIN, None)


@functools.lru_cache(maxsize=None)
def inputs(key, l):
    S = solver(*key)
    L, n, dim = S.levels[l], S.n, S.dim
    rng = np.random.default_rng(500 + l)
    fs = L.P * pu.face_size(n, dim)
    u = rng.uniform(-1.0, 1.0, fs)
    u[rng.random(fs) < 0.05] = 0.0
    d = types.SimpleNamespace(c=rng.uniform(0.5, 2.0, L.size), cb=rng.uniform(0.5, 2.0, pu.num_bfaces(L) * L.nf),
                              U=pu.pack(*au.single_valued(L, pu.unpack(u, n, dim))), W=util.rand_vec(fs, 510 + l))
    for v in vars(d).values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def statement(key, l, with_cb):
    S, d = solver(*key), inputs(key, l)
    return pu.pack(*au.advect_flux(S.levels[l], pu.unpack(d.U, S.n, S.dim), d.c, d.cb if with_cb else None))


def run(S, l, with_cb, fused=True):
    """the device's flux, fused update and composed update of level l"""
    g, d = S.g, inputs(S.key, l)
    dU, dc, dcb = g.new_face_vector(l, d.U), g.new_vector(l, d.c), g.new_boundary_vector(l, d.cb if d.cb.size else None)
    b = dcb if with_cb else None
    dF, out, comp, dd = g.new_face_vector(l), g.new_vector(l), g.new_vector(l), g.new_vector(l)
    dF.set(-7.0)
    out.set(-7.0)
    g.advect_flux(dU, dc, dF, cb=b, level=l)
    g.advect(dU, dc, out, alpha=ALPHA, cb=b, level=l)
    g.divergence(dF, dd, alpha=ALPHA, level=l)
    comp.copy(dc)
    comp.addScaled(-1.0, dd)
    return dF.download(), out.download(), comp.download()


@pytest.mark.parametrize("name,div,mask,n,dim", CASES, ids=IDS)
def test_against_the_statement_and_fused_equals_composed(name, div, mask, n, dim):
    S = solver(name, div, mask, n, dim)
    g = S.g
    assert len(S.levels) >= 2
    for l, L in enumerate(S.levels):
        d = inputs(S.key, l)
        for with_cb in (False, True):
            F, fused, comp = run(S, l, with_cb)
            want = statement(S.key, l, with_cb)
            bad = np.nonzero(fused != comp)[0] % n ** dim  # (which cells of a patch, should the two ever differ: x and y parity)
            print(f"level {l} cb={with_cb}: flux differs in {int((F != want).sum())} entries, fused in {bad.size} cells",
                  np.unique(bad % 2 + 2 * (bad // n % 2), return_counts=True) if bad.size else "")
            assert np.array_equal(F, want), (l, with_cb, np.abs(F - want).max())
            assert np.array_equal(fused, comp), (l, with_cb, np.abs(fused - comp).max(), int((fused != comp).sum()))
            assert not np.array_equal(fused, d.c)
            # the flux is a fixed point of the matching
            dF = g.new_face_vector(l, F)
            g.faces_match(dF, level=l)
            assert np.array_equal(dF.download(), F), (l, with_cb)
        # te_faces_match on a face field whose copies agree nowhere; te_faces_max_rate
        dW = g.new_face_vector(l, d.W)
        g.faces_match(dW, level=l)
        assert np.array_equal(dW.download(), pu.pack(*au.faces_match(L, pu.unpack(d.W, n, dim)))), l
        for a in (d.U, d.W):
            assert g.faces_max_rate(g.new_face_vector(l, a), level=l) == au.max_rate(L, pu.unpack(a, n, dim)), l


@pytest.mark.parametrize("name,n,zs", SLABS, ids=[f"{c[0]}-n{c[1]}-zs{c[2]}" for c in SLABS])
def test_every_slab_instantiation_gives_the_bits_of_one_slab(name, n, zs):
    S = solver(name, 1 if name == "uniform" else 0, bc_util.CHANNEL, n, 3)
    base = slab_run(S.key, 1)
    got = slab_run(S.key, zs)
    for k in base:
        assert np.array_equal(got[k], base[k]), k


@functools.lru_cache(maxsize=None)
def slab_run(key, zs):
    S = solver(*key)
    out = {}
    with pinned(S.g, zs):
        for l in range(len(S.levels)):
            out[l, "flux"], out[l, "fused"], _ = run(S, l, True)
    return out


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
        rate = g.faces_max_rate(dU, level=l)
        alpha = 0.9 / (dim * rate)
        g.advect_flux(dU, dc, dF, level=l)
        g.advect(dU, dc, out, alpha=alpha, level=l)
        total = abs(math.fsum(((out.download() - c) * au.cell_volumes(L)).tolist()))
        bound = 16 * EPS * alpha * au.flux_area_sum(L, pu.unpack(dF.download(), n, dim))
        print(f"level {l}: imbalance {total:.3e}, {total / bound:.3f} of the bound")
        assert total <= bound, (l, total, bound)
        # positivity: alpha dim rate = 1 for a one-way velocity, alpha 2 dim rate = 1 for any (tests/test_advect_host.py)
        for U, factor in ((pu.pack(*au.one_way(pu.unpack(d.U, n, dim))), dim), (d.U, 2 * dim)):
            dU.upload(U)
            a = 1.0 / (factor * g.faces_max_rate(dU, level=l))
            for b in (None, dcb):
                g.advect(dU, dc, out, alpha=a, cb=b, level=l)
                assert out.download().min() >= 0.0, (l, factor)


def test_profile_rows_name_the_four_classes():
    S = solver("2refine.bin", 0, 0, 4, 3)
    g, d = S.g, inputs(S.key, 0)
    dU, dF = g.new_face_vector(0, d.U), g.new_face_vector(0)
    g.profile(True)
    g.profile_reset()
    g.advect_flux(dU, g.new_vector(0, d.c), dF)
    g.advect(dU, g.new_vector(0, d.c), g.new_vector(0))
    g.faces_match(dF)
    g.faces_max_rate(dU)
    rows = g.profile_rows()
    g.profile(False)
    for k in ("advect_flux", "advect"):
        assert k in rows and rows[k]["calls"] == 1 and rows[k]["cells"] == S.H.cells(0), (k, sorted(rows))
    assert rows["faces_match"]["calls"] == 1 and rows["faces_match"]["cells"] > 0
    assert rows["faces_max_rate"]["calls"] == 1 and rows["faces_max_rate"]["cells"] == d.U.size
    assert rows["cf_ghost"]["calls"] == 2  # the flux slots, once per call


@pytest.mark.parametrize("key", [("2refine.bin", 0, bc_util.CHANNEL, 8, 3), ("2d2ref.bin", 0, bc_util.MASKS2[0], 8, 2)], ids=["3d", "2d"])
def test_the_calls_leave_the_solver_as_it_was(key):
    S = solver(*key)
    g = S.g
    f = g.new_vector(0, util.rand_vec(S.levels[0].size, 3))
    o = g.default_opts(smoother=capi.SMOOTH_RBGS)  # V(1,1)

    def cycle_bits():
        u = g.new_vector(0)
        g.cycle(o, f, u)
        return u.download()

    before = cycle_bits()
    for l in range(g.num_levels):
        d = inputs(S.key, l)
        dU, dF = g.new_face_vector(l, d.U), g.new_face_vector(l)
        g.advect_flux(dU, g.new_vector(l, d.c), dF, cb=g.new_boundary_vector(l, d.cb), level=l)
        g.advect(dU, g.new_vector(l, d.c), g.new_vector(l), alpha=0.5, level=l)
        g.faces_match(dF, level=l)
        g.faces_max_rate(dU, level=l)
    assert not g.has_coefficient() and not g.has_reaction()
    assert np.array_equal(cycle_bits(), before)
    # the flux slots right in front of an operator application: te_apply refills the ghost slots it reads
    d = inputs(S.key, 0)
    u, A0, A1 = g.new_vector(0, d.c), g.new_vector(0), g.new_vector(0)
    g.apply(u, A0)
    g.advect(g.new_face_vector(0, d.U), u, g.new_vector(0))
    g.apply(u, A1)
    assert np.array_equal(A0.download(), A1.download())


def test_refusals():
    S, S2 = solver("2refine.bin", 0, bc_util.CHANNEL, 4, 3), solver("uniform", 2, bc_util.CHANNEL, 4, 3)
    g, g2 = S.g, S2.g
    c, c2, c1, U, F, F1, b, b1, i = (g.new_vector(0), g.new_vector(0), g.new_vector(1), g.new_face_vector(0), g.new_face_vector(0), g.new_face_vector(1),
                                     g.new_boundary_vector(0), g.new_boundary_vector(1), g.new_iface_vector(0))
    oc, oF, ob = g2.new_vector(0), g2.new_face_vector(0), g2.new_boundary_vector(0)
    lib, NULL = capi.lib(), None
    rate = capi.C.c_double(0.0)
    einval = [
        # te_advect_flux: NULL, aliasing, wrong kind, level, solver
        lambda: capi.check(lib.te_advect_flux(g.h, 0, NULL, c.h, NULL, F.h)), lambda: capi.check(lib.te_advect_flux(g.h, 0, U.h, NULL, NULL, F.h)),
        lambda: capi.check(lib.te_advect_flux(g.h, 0, U.h, c.h, NULL, NULL)), lambda: capi.check(lib.te_advect_flux(NULL, 0, U.h, c.h, NULL, F.h)),
        lambda: g.advect_flux(U, c, U), lambda: g.advect_flux(c, c, F), lambda: g.advect_flux(U, F, F), lambda: g.advect_flux(U, c, c),
        lambda: g.advect_flux(U, b, F), lambda: g.advect_flux(U, i, F), lambda: g.advect_flux(U, c, F, cb=c), lambda: g.advect_flux(U, c, F, cb=i),
        lambda: g.advect_flux(F1, c, F), lambda: g.advect_flux(U, c1, F), lambda: g.advect_flux(U, c, F1), lambda: g.advect_flux(U, c, F, cb=b1),
        lambda: g.advect_flux(U, c, F, level=1), lambda: g.advect_flux(U, c, F, level=-1), lambda: g.advect_flux(U, c, F, level=g.num_levels),
        lambda: g.advect_flux(oF, c, F), lambda: g.advect_flux(U, oc, F), lambda: g.advect_flux(U, c, oF), lambda: g.advect_flux(U, c, F, cb=ob),
        # te_advect
        lambda: capi.check(lib.te_advect(g.h, 0, 1.0, NULL, c.h, NULL, c2.h)), lambda: capi.check(lib.te_advect(g.h, 0, 1.0, U.h, NULL, NULL, c2.h)),
        lambda: capi.check(lib.te_advect(g.h, 0, 1.0, U.h, c.h, NULL, NULL)), lambda: capi.check(lib.te_advect(NULL, 0, 1.0, U.h, c.h, NULL, c2.h)),
        lambda: g.advect(U, c, c), lambda: g.advect(c, c, c2), lambda: g.advect(U, F, c2), lambda: g.advect(U, c, F), lambda: g.advect(U, c, b),
        lambda: g.advect(U, c, c2, cb=F), lambda: g.advect(F1, c, c2), lambda: g.advect(U, c1, c2), lambda: g.advect(U, c, c1),
        lambda: g.advect(U, c, c2, cb=b1), lambda: g.advect(U, c, c2, level=1), lambda: g.advect(oF, c, c2), lambda: g.advect(U, oc, c2),
        lambda: g.advect(U, c, oc), lambda: g.advect(U, c, c2, cb=ob),
        # te_faces_match, te_faces_max_rate
        lambda: capi.check(lib.te_faces_match(g.h, 0, NULL)), lambda: capi.check(lib.te_faces_match(NULL, 0, F.h)), lambda: g.faces_match(c),
        lambda: g.faces_match(b), lambda: g.faces_match(F1), lambda: g.faces_match(F, level=1), lambda: g.faces_match(oF),
        lambda: capi.check(lib.te_faces_max_rate(g.h, 0, NULL, capi.C.byref(rate))), lambda: capi.check(lib.te_faces_max_rate(g.h, 0, U.h, NULL)),
        lambda: g.faces_max_rate(c), lambda: g.faces_max_rate(b), lambda: g.faces_max_rate(F1), lambda: g.faces_max_rate(U, level=1),
        lambda: g.faces_max_rate(oF),
    ]
    for k, call in enumerate(einval):
        with pytest.raises(capi.TeError) as e:
            call()
        assert e.value.code == capi.TE_EINVAL, k


def test_a_sharded_hierarchy_is_refused_and_still_cycles():
    """two virtual ranks with a fabric attached: the four calls answer TE_ESTATE ("sharded"), a DIRECT cycle runs afterwards"""
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
        for call in (lambda: g.advect_flux(U, c, F), lambda: g.advect(U, c, out), lambda: g.faces_match(F), lambda: g.faces_max_rate(U)):
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
        assert seen == [(capi.TE_ESTATE, True)] * 4, seen
    assert max(norm for _, norm in outs) > 0.0
