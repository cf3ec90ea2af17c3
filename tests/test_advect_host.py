"""CPU: the numpy statement of the transport calls (tests/advect_util.py, the specification of te_advect_flux, te_advect,
te_faces_match and te_faces_max_rate) on its own, and the surface the feature adds.

Bounds (none of them comes from what the device gives):
  conservation   |sum_cells (out - c) volume| <= 16 eps alpha sum_entries |F| area, the sum over the stored entries of the statement's
                 own flux: every flux enters two cells with opposite signs, and a cell's sum rounds at most 2 dim + 1 times. The sum
                 over the cells is taken exactly (math.fsum). On 2refine.bin / 2d2ref.bin this is the test of the matching: without the
                 coarse-side mean (advect_util's match=False) the same statement must FAIL there.
  positivity     c >= 0, cb >= 0: out >= 0 in every cell (DESIGN.md 23 proves both) with alpha = 1 / (dim rate) for a velocity that
                 leaves no cell through both of its faces along an axis (advect_util.one_way: a cell's outflow rates then sum to at
                 most dim rate, as they do for a discretely divergence-free field), and with alpha = 1 / (2 dim rate) for any
                 velocity whatever (a random one makes some cell a source along every axis, and alpha dim rate = 1 is then NOT enough)
  faces_match    idempotent and the identity on advect_flux's output: bit for bit"""
import math

import numpy as np
import pytest

from pressurepoissonsolver_amd import capi
from tests import advect_util as au, bc_util, density_util as du, projection_util as pu, util

EPS = util.EPS
# (mesh, n, divides, dim): the shapes of tests/test_gpu_advect.py
SHAPES = [("uniform", 4, 2, 3), ("uniform", 8, 2, 3), ("uniform", 32, 1, 3), ("2refine.bin", 4, 0, 3), ("2refine.bin", 16, 0, 3),
          ("uniform", 8, 3, 2), ("2d2ref.bin", 8, 0, 2)]
REFINED = [s for s in SHAPES if s[0].endswith(".bin")]
IDS = lambda v: str(v)


def fields(L, seed, zero_physical=False):
    """c > 0, cb > 0 and a single-valued U with both signs and some exact zeros"""
    rng = np.random.default_rng(seed)
    n, dim = L.n, L.dim
    c = rng.uniform(0.5, 2.0, L.size)
    cb = rng.uniform(0.5, 2.0, pu.num_bfaces(L) * L.nf)
    u = rng.uniform(-1.0, 1.0, L.P * pu.face_size(n, dim))
    u[rng.random(u.size) < 0.05] = 0.0
    return c, cb, au.single_valued(L, pu.unpack(u, n, dim), zero_physical)


def levels_of(name, n, div, dim, mask=0):
    return bc_util.setup(name, n, div, mask, dim)[2]


def test_the_surface_has_the_four_calls():
    for name in ("te_advect_flux", "te_advect", "te_faces_match", "te_faces_max_rate"):
        assert name in capi.SYMBOLS, name
    for method in ("advect_flux", "advect", "faces_match", "faces_max_rate"):
        assert callable(getattr(capi.GMG, method, None)), method
    import ctypes
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("te_advect_flux", "te_advect", "te_faces_match", "te_faces_max_rate"):
        assert hasattr(lib, name), name


def imbalance(L, U, c, alpha, cb, match=True):
    out, F = au.advect(L, U, c, alpha, cb, match)
    total = math.fsum(((out - c) * au.cell_volumes(L)).tolist())
    return abs(total), 16 * EPS * alpha * au.flux_area_sum(L, F)


@pytest.mark.parametrize("name,n,div,dim", SHAPES, ids=IDS)
def test_the_update_conserves(name, n, div, dim):
    for l, L in enumerate(levels_of(name, n, div, dim)):
        c, cb, U = fields(L, 40 + l, zero_physical=True)
        alpha = 0.9 / (dim * au.max_rate(L, U))
        for b in (None, cb):
            got, bound = imbalance(L, U, c, alpha, b)
            print(f"{name} n={n} level {l}: imbalance {got:.3e}, {got / bound:.3f} of the bound")
            assert got <= bound, (l, got, bound)


@pytest.mark.parametrize("name,n,div,dim", REFINED, ids=IDS)
def test_without_the_coarse_side_mean_conservation_fails(name, n, div, dim):
    L = levels_of(name, n, div, dim)[0]
    assert (L.a["nbr_kind"] == 3).any()
    c, cb, U = fields(L, 40, zero_physical=True)
    alpha = 0.9 / (dim * au.max_rate(L, U))
    got, bound = imbalance(L, U, c, alpha, None, match=False)
    print(f"{name} n={n}: unmatched imbalance {got:.3e} against the bound {bound:.3e}")
    assert got > bound


@pytest.mark.parametrize("field", ["one_way", "any"])
@pytest.mark.parametrize("name,n,div,dim", SHAPES, ids=IDS)
def test_the_update_keeps_a_field_non_negative(name, n, div, dim, field):
    mask = bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0]
    for l, L in enumerate(levels_of(name, n, div, dim, mask)):
        c, cb, U = fields(L, 50 + l)
        c = np.where(np.random.default_rng(7).random(c.size) < 0.2, 0.0, c)  # some cells hold exactly nothing
        # alpha dim rate = 1 where a cell's outflow rates sum to at most dim rate; any U at all: they sum to at most 2 dim rate
        U = au.one_way(U) if field == "one_way" else U
        alpha = 1.0 / ((dim if field == "one_way" else 2 * dim) * au.max_rate(L, U))
        for b in (None, cb):
            out, _ = au.advect(L, U, c, alpha, b)
            assert out.min() >= 0.0, (l, out.min())
        assert not np.array_equal(out, c)


@pytest.mark.parametrize("name,n,div,dim", SHAPES, ids=IDS)
def test_faces_match_is_idempotent_and_leaves_a_flux_alone(name, n, div, dim):
    for l, L in enumerate(levels_of(name, n, div, dim)):
        c, cb, U = fields(L, 60 + l)
        once = au.faces_match(L, U)
        twice = au.faces_match(L, once)
        assert np.array_equal(pu.pack(*once), pu.pack(*twice)), l
        changed = not np.array_equal(pu.pack(*once), pu.pack(*U))
        assert changed == bool((L.a["nbr_kind"] == 3).any()), l  # it does something exactly where there is a coarse/fine face
        F = au.advect_flux(L, U, c, cb)
        assert np.array_equal(pu.pack(*au.faces_match(L, F)), pu.pack(*F)), l
        # both copies of a same-level face of the flux agree, since U's do
        for p, a, q in du.same_level_pairs(L):
            assert np.array_equal(F[1][p, a], du.lower_face(F[0], q, a, dim)), (l, p, a)


def test_max_rate_is_the_largest_entry_over_its_spacing():
    L = levels_of("2refine.bin", 4, 0, 3)[0]
    U = pu.unpack(np.zeros(L.P * pu.face_size(4, 3)), 4, 3)
    assert au.max_rate(L, U) == 0.0
    p = int(np.argmin(L.a["h"][:, 1]))
    U[1][p, 1][2, 1] = -3.0
    assert au.max_rate(L, U) == 3.0 / L.a["h"][p, 1]
