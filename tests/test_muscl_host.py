"""CPU: the numpy statement of the second-order transport calls (tests/muscl_util.py, the specification of te_cell_slopes,
te_advect_flux_muscl and te_advect_muscl) on its own, and the surface the feature adds.

Bounds (none of them comes from what the device gives):
  ZERO           the flux of tests/advect_util.py bit for bit: c + 0.5 * 0.0 is c
  conservation   |sum_cells (out - c) volume| <= 16 eps alpha sum_entries |F| area, section 23's statement and bound, U single-valued
                 and zero on the physical faces. Without the coarse-side mean (match=False) the same statement must FAIL.
  positivity     c >= 0, cb >= 0, ANY U: out >= 0 with alpha K dim rate = 1, K = muscl_util.positivity_factor: 2 on a level without
                 coarse/fine faces (each edge state lies between the cell and a neighbour, hence >= 0, and the two edge states of a
                 cell along an axis sum to 2c), 2.5 on a level with them: a coarse cell loses its RAW value through a coarse/fine face,
                 at half the rate, beside up to 2c through the opposite face. test_two_dim_rate_is_not_enough_beside_a_coarse_fine_face
                 builds that cell: with K = 2 it goes negative under MC, with K = 2.5 it does not. CENTRAL has no such bound and must
                 go negative on one of the random inputs (seed 50 + level, found on the CPU: 2refine.bin n = 4, level 0).
  order          log2 of the L1 error ratio 32^2 -> 64^2 of a Gaussian bump moved by U = (1, 0.5) to T = 0.25 with Heun steps:
                 <= 1.0 for ZERO, >= 1.5 for MC, >= 1.8 for CENTRAL, and MC's error at 64^2 at most a fifth of ZERO's. The thresholds
                 only separate first from second order."""
import functools
import math

import numpy as np
import pytest

from pressurepoissonsolver_amd import capi
from tests import advect_util as au, bc_util, density_util as du, muscl_util as mu, projection_util as pu, util
from tests.test_advect_host import fields, levels_of

EPS = util.EPS
REFINED = [("2refine.bin", 4, 0, 3), ("2d2ref.bin", 8, 0, 2)]
IDS = lambda v: str(v)
KIND_NAMES = {mu.ZERO: "zero", mu.MINMOD: "minmod", mu.MC: "mc", mu.CENTRAL: "central"}


def test_the_surface_has_the_three_calls():
    names = ("te_cell_slopes", "te_advect_flux_muscl", "te_advect_muscl")
    for name in names:
        assert name in capi.SYMBOLS, name
    for method in ("cell_slopes", "advect_flux_muscl", "advect_muscl"):
        assert callable(getattr(capi.GMG, method, None)), method
    assert (capi.SLOPE_ZERO, capi.SLOPE_MINMOD, capi.SLOPE_MC, capi.SLOPE_CENTRAL) == mu.KINDS == (0, 1, 2, 3)
    import ctypes
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), name


def test_the_slope_kinds_on_known_differences():
    dm = np.array([1.0, 1.0, -2.0, 1.0, 0.0, 3.0, -1.0])
    dp = np.array([3.0, 0.5, -1.0, -1.0, 2.0, 1.0, -8.0])
    assert np.array_equal(mu.slope(mu.ZERO, dm, dp), np.zeros(7))
    assert np.array_equal(mu.slope(mu.MINMOD, dm, dp), [1.0, 0.5, -1.0, 0.0, 0.0, 1.0, -1.0])
    assert np.array_equal(mu.slope(mu.MC, dm, dp), [2.0, 0.75, -1.5, 0.0, 0.0, 2.0, -2.0])
    assert np.array_equal(mu.slope(mu.CENTRAL, dm, dp), [2.0, 0.75, -1.5, 0.0, 1.0, 2.0, -4.5])
    for kind in (mu.MINMOD, mu.MC):  # |S| <= 2 min(|dm|, |dp|), with the sign of both
        rng = np.random.default_rng(3)
        a, b = rng.uniform(-1, 1, 4000), rng.uniform(-1, 1, 4000)
        S = mu.slope(kind, a, b)
        assert (np.abs(S) <= 2 * np.minimum(np.abs(a), np.abs(b))).all() and (S * a >= 0).all() and (S * b >= 0).all()


@pytest.mark.parametrize("name,n,div,dim", REFINED, ids=IDS)
def test_zero_slopes_give_the_donor_cell_flux(name, n, div, dim):
    for l, L in enumerate(levels_of(name, n, div, dim)):
        c, cb, U = fields(L, 30 + l)
        for b in (None, cb):
            assert not mu.cell_slopes(L, c, mu.ZERO, b).any()
            assert np.array_equal(pu.pack(*mu.advect_flux(L, U, c, mu.ZERO, b)), pu.pack(*au.advect_flux(L, U, c, b))), l
            assert not np.array_equal(pu.pack(*mu.advect_flux(L, U, c, mu.MC, b)), pu.pack(*au.advect_flux(L, U, c, b))), l


def imbalance(L, U, c, alpha, kind, cb, match=True):
    out, F = mu.advect(L, U, c, alpha, kind, cb, match)
    total = math.fsum(((out - c) * au.cell_volumes(L)).tolist())
    return abs(total), 16 * EPS * alpha * au.flux_area_sum(L, F)


@pytest.mark.parametrize("kind", [mu.MINMOD, mu.MC], ids=KIND_NAMES.get)
@pytest.mark.parametrize("name,n,div,dim", REFINED, ids=IDS)
def test_the_update_conserves_and_fails_to_without_the_coarse_side_mean(name, n, div, dim, kind):
    for l, L in enumerate(levels_of(name, n, div, dim)):
        c, cb, U = fields(L, 40 + l, zero_physical=True)
        alpha = 0.9 / (dim * au.max_rate(L, U))
        for b in (None, cb):
            got, bound = imbalance(L, U, c, alpha, kind, b)
            print(f"{name} n={n} level {l}: imbalance {got:.3e}, {got / bound:.3f} of the bound")
            assert got <= bound, (l, got, bound)
        if l == 0:  # the negative control
            assert (L.a["nbr_kind"] == 3).any()
            got, bound = imbalance(L, U, c, alpha, kind, None, match=False)
            print(f"{name} n={n}: unmatched imbalance {got:.3e} against the bound {bound:.3e}")
            assert got > bound


@pytest.mark.parametrize("name,n,div,dim", REFINED, ids=IDS)
def test_the_flux_is_a_fixed_point_of_the_matching(name, n, div, dim):
    for l, L in enumerate(levels_of(name, n, div, dim)):
        c, cb, U = fields(L, 60 + l)
        for kind in mu.KINDS:
            F = mu.advect_flux(L, U, c, kind, cb)
            assert np.array_equal(pu.pack(*au.faces_match(L, F)), pu.pack(*F)), (l, kind)
            # both copies of a same-level face of the flux agree, since U's do
            for p, a, q in du.same_level_pairs(L):
                assert np.array_equal(F[1][p, a], du.lower_face(F[0], q, a, dim)), (l, p, a)


def positivity_inputs(L, l):
    """random U with both signs and exact zeros, c >= 0 with 20 % exact zeros, cb > 0"""
    c, cb, U = fields(L, 50 + l)
    return np.where(np.random.default_rng(7).random(c.size) < 0.2, 0.0, c), cb, U


def test_limited_slopes_keep_a_field_non_negative_and_central_does_not():
    central_min = 0.0
    for name, n, div, dim in REFINED:
        mask = bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0]
        for l, L in enumerate(levels_of(name, n, div, dim, mask)):
            c, cb, U = positivity_inputs(L, l)
            alpha = 1.0 / (mu.positivity_factor(L) * dim * au.max_rate(L, U))
            for b in (None, cb):
                for kind in mu.LIMITED:
                    out, _ = mu.advect(L, U, c, alpha, kind, b)
                    assert out.min() >= 0.0, (name, l, kind, out.min())
                    assert not np.array_equal(out, c)
                lowest = mu.advect(L, U, c, alpha, mu.CENTRAL, b)[0].min()
                print(f"{name} level {l} cb={b is not None}: CENTRAL's minimum {lowest:.3e}")
                central_min = min(central_min, lowest)
    assert central_min < 0.0  # the negative control: the unlimited slope has no such bound


def set_face(lo, hi, n, p, a, idx, upper, v):
    """U on the lower / upper a-face of cell idx (array order) of patch p <- v"""
    ax = len(idx) - 1 - a
    idx = list(idx)
    if not upper:
        lo[p, a][tuple(idx)] = v
    elif idx[ax] < n - 1:
        idx[ax] += 1
        lo[p, a][tuple(idx)] = v
    else:
        del idx[ax]
        hi[p, a][tuple(idx)] = v


def worst_coarse_cell(L):
    """2D. A coarse cell beside a coarse/fine face with outflow through all four faces at the level's rate: the fine cells beyond the
    coarse/fine face hold 0, the cell 1, its neighbour on the other side 4 (MC: S = 2, the edge state there 2c) -> the cell loses
    0.5 c + 2c along that axis and 2c along the other: 4.5 c rate"""
    n, dim = L.n, L.dim
    assert dim == 2
    kind, nbr, h = L.a["nbr_kind"], L.a["nbr"], L.a["h"]
    p, s = next((p, s) for p in range(L.P) for s in range(4) if kind[p, s] == 3)
    a, upper = s >> 1, s & 1
    ax, j = dim - 1 - a, 1  # face coordinate 1 lies in the first half: the fine patch is nbr[p, s, 0], its faces 2 and 3
    f = int(nbr[p, s, 0])
    C = np.zeros((L.P, n, n))
    cell, inner = [j, j], [j, j]
    cell[ax], inner[ax] = (n - 1, n - 2) if upper else (0, 1)
    C[p][tuple(cell)], C[p][tuple(inner)] = 1.0, 4.0
    lo, hi = pu.unpack(np.zeros(L.P * pu.face_size(n, dim)), n, dim)
    rate = 1.0
    out_sign = 1.0 if upper else -1.0
    for t in (2 * j, 2 * j + 1):  # the fine copies of the coarse/fine face, outward from the coarse cell
        fcell = [t, t]
        fcell[ax] = 0 if upper else n - 1
        set_face(lo, hi, n, f, a, fcell, not upper, out_sign * rate * h[f, a])
    set_face(lo, hi, n, p, a, cell, not upper, -out_sign * rate * h[p, a])  # the opposite face, outward
    set_face(lo, hi, n, p, 1 - a, cell, 0, -rate * h[p, 1 - a])
    set_face(lo, hi, n, p, 1 - a, cell, 1, rate * h[p, 1 - a])
    at = p * n * n + cell[0] * n + cell[1]
    return C.ravel(), (lo, hi), at


def test_two_dim_rate_is_not_enough_beside_a_coarse_fine_face():
    L = levels_of("2d2ref.bin", 8, 0, 2)[0]
    c, U, at = worst_coarse_cell(L)
    rate = au.max_rate(L, U)
    assert rate == 1.0 and mu.positivity_factor(L) == 2.5
    two = mu.advect(L, U, c, 1.0 / (2 * 2 * rate), mu.MC)[0]
    safe = mu.advect(L, U, c, 1.0 / (2.5 * 2 * rate), mu.MC)[0]
    print(f"the cell under alpha 2 dim rate = 1: {two[at]:.4f}; under alpha 2.5 dim rate = 1: {safe[at]:.4f}")
    assert two[at] == 1.0 - 4.5 / 4 and two.min() < 0.0
    assert abs(safe[at] - 0.1) < 1e-15 and safe.min() >= 0.0
    for kind in (mu.ZERO, mu.MINMOD):  # these two lose at most 1.5 c and 2c along the axis: 2 dim is enough for them even here
        assert mu.advect(L, U, c, 1.0 / (2 * 2 * rate), kind)[0].min() >= 0.0


# ---- order: a Gaussian bump of width 0.07 moved by U = (1, 0.5) for T = 0.25, Heun steps with alpha = 0.25 h
WIDTH, CENTRE, VEL, T_END = 0.07, (0.35, 0.4), (1.0, 0.5), 0.25
ORDER_MESHES = {32: ("uniform", 2, 8, 2), 64: ("uniform", 3, 8, 2)}  # (name, divides, n, dim): 8^2 patches


def bump(L, starts, shift):
    """the bump at the cell centres of a 2D level, its centre moved by VEL * shift"""
    n, h = L.n, L.a["h"]
    out = np.zeros((L.P, n, n))
    for p in range(L.P):
        x = starts[p, 0] + (np.arange(n) + 0.5) * h[p, 0] - (CENTRE[0] + VEL[0] * shift)
        y = starts[p, 1] + (np.arange(n) + 0.5) * h[p, 1] - (CENTRE[1] + VEL[1] * shift)
        out[p] = np.exp(-(x[None, :] ** 2 + y[:, None] ** 2) / (2 * WIDTH ** 2))
    return out.ravel()


def constant_velocity(L):
    lo, hi = pu.unpack(np.zeros(L.P * pu.face_size(L.n, 2)), L.n, 2)
    for a in range(2):
        lo[:, a] = VEL[a]
        hi[:, a] = VEL[a]
    return lo, hi


@functools.lru_cache(maxsize=None)
def order_problem(cells):
    name, div, n, dim = ORDER_MESHES[cells]
    m, H, levels = bc_util.setup(name, n, div, 0, dim)
    L = levels[0]
    starts = H.tables(0)["starts"]
    h = float(L.a["h"][0, 0])
    assert L.P * n * n == cells * cells and np.all(L.a["h"][:, :2] == h)
    steps = int(round(T_END / (0.25 * h)))
    assert steps == cells
    return H, L, bump(L, starts, 0.0), bump(L, starts, T_END), 0.25 * h, steps


def heun(adv, c, steps):
    for _ in range(steps):
        c = 0.5 * (c + adv(adv(c)))
    return c


@functools.lru_cache(maxsize=None)
def statement_run(cells, kind):
    """the statement's field at T_END and its L1 error"""
    H, L, c0, exact, alpha, steps = order_problem(cells)
    U = constant_velocity(L)
    c = heun(lambda v: mu.advect(L, U, v, alpha, kind)[0], c0, steps)
    c.setflags(write=False)
    return c, float(np.abs(c - exact).mean())


def order_gates(err):
    """err[kind][cells] -> the five gates of the order test, printed with their values"""
    order = {k: math.log2(err[k][32] / err[k][64]) for k in err}
    ratio = err[mu.MC][64] / err[mu.ZERO][64]
    for k in err:
        print(f"{KIND_NAMES[k]:8s} L1 error {err[k][32]:.3e} (32^2), {err[k][64]:.3e} (64^2), order {order[k]:.3f}")
    print(f"MC / ZERO at 64^2: {ratio:.4f} (1/{1 / ratio:.1f})")
    assert order[mu.ZERO] <= 1.0, order
    assert order[mu.MC] >= 1.5, order
    assert order[mu.CENTRAL] >= 1.8, order
    assert ratio <= 0.2, ratio
    return order, ratio


def test_order_of_accuracy():
    err = {k: {cells: statement_run(cells, k)[1] for cells in (32, 64)} for k in (mu.ZERO, mu.MC, mu.CENTRAL)}
    order_gates(err)
    assert statement_run(64, mu.MC)[0].min() >= 0.0  # (the limited field never goes negative)
    assert statement_run(32, mu.CENTRAL)[0].min() < 0.0  # (the unlimited one does)
