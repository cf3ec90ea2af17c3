"""CPU: the numpy statement of the variable-density step (tests/density_util.py, the specification of te_faces_from_cells,
te_project_weighted and te_add_boundary_rhs_weighted) on its own, and the surface the feature adds.

Bounds (none of them comes from what the device gives):
  symmetry            both copies of a same-level face: bit for bit (the same operands; + and * commute)
  coarse/fine, MEAN   coarse copy against the mean of the fine copies: 4 eps max|c| (the same eight cells in another association)
  constant field      MEAN and RECIP_MEAN exact; HARMONIC 2 eps relative (c0 c0 rounds once, the quotient once)
  weighted fold       against -div(w (.) grad(0, bd)): 16 eps dim 2 max(w) max|bd| / h_min^2 (up to dim terms of size 2 w |bd| / h^2 per
                      cell, each a few roundings in either form)
  order               consecutive max-error ratios >= 3.5 (second order: 4 in the limit), test_varcoef_host.py's convention"""
import numpy as np
import pytest

from pressurepoissonsolver_amd import capi
from tests import bc_util, density_util as du, projection_util as pu, prolong_util, util, varcoef_util as vc

EPS = util.EPS
MESHES = [("2refine.bin", 4, 0, 3), ("2d2ref.bin", 8, 1, 2), ("uniform", 4, 2, 3), ("uniform", 8, 2, 2)]


def positive(size, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, size)


def test_the_surface_has_the_three_calls():
    for name in ("te_faces_from_cells", "te_project_weighted", "te_add_boundary_rhs_weighted"):
        assert name in capi.SYMBOLS, name
    for method in ("faces_from_cells", "project_weighted", "add_boundary_rhs_weighted"):
        assert callable(getattr(capi.GMG, method, None)), method
    assert (capi.FACE_MEAN, capi.FACE_HARMONIC, capi.FACE_RECIP_MEAN) == (0, 1, 2) == du.MODES
    import ctypes
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("te_faces_from_cells", "te_project_weighted", "te_add_boundary_rhs_weighted"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name,n,div,dim", MESHES, ids=lambda v: str(v))
def test_same_level_copies_are_equal_bit_for_bit(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    for l, L in enumerate(levels):
        c = positive(L.size, 10 + l)
        pairs = du.same_level_pairs(L)
        assert pairs or L.P == 1
        for mode in du.MODES:
            lo, hi = du.faces_from_cells(L, c, mode)
            for p, a, q in pairs:
                assert np.array_equal(hi[p, a], du.lower_face(lo, q, a, dim)), (l, mode, p, a)


@pytest.mark.parametrize("name,n,div,dim", [("2refine.bin", 4, 0, 3), ("2d2ref.bin", 8, 0, 2)], ids=lambda v: str(v))
def test_coarse_copy_is_the_mean_of_the_fine_copies(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    L = levels[0]
    c = positive(L.size, 3)
    lo, hi = du.faces_from_cells(L, c, du.MEAN)
    kind, nbr = L.a["nbr_kind"], L.a["nbr"]
    h, seen = n // 2, 0
    for p in range(L.P):
        for s in range(2 * dim):
            if kind[p, s] != 3:
                continue
            seen += 1
            coarse = du.side_face(lo, hi, p, s, dim)
            mean = np.zeros_like(coarse)
            for qd in range(1 << (dim - 1)):
                F = du.side_face(lo, hi, int(nbr[p, s, qd]), s ^ 1, dim)
                assert L.a["nbr_kind"][int(nbr[p, s, qd]), s ^ 1] == 2
                qa, qb = qd & 1, qd >> 1
                if dim == 2:
                    mean[qa * h:(qa + 1) * h] = (F[0::2] + F[1::2]) * 0.5
                else:
                    mean[qb * h:(qb + 1) * h, qa * h:(qa + 1) * h] = ((F[0::2, 0::2] + F[0::2, 1::2]) + (F[1::2, 0::2] + F[1::2, 1::2])) * 0.25
            err = np.abs(coarse - mean).max()
            assert err <= 4 * EPS * np.abs(c).max(), (p, s, err)
    assert seen > 0


@pytest.mark.parametrize("name,n,div,dim", MESHES, ids=lambda v: str(v))
def test_a_constant_field_gives_the_constant_on_every_face(name, n, div, dim):
    m, H, levels = bc_util.setup(name, n, div, bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0], dim)
    c0 = 1.7320508075688772
    for l, L in enumerate(levels):
        c = np.full(L.size, c0)
        kinds = set(L.a["nbr_kind"].ravel().tolist())
        assert 0 in kinds and (not name.endswith(".bin") or l > 0 or {2, 3} <= kinds)
        for cb in (None, np.full(pu.num_bfaces(L) * L.nf, c0)):
            for mode in du.MODES:
                lo, hi = du.faces_from_cells(L, c, mode, cb)
                got = np.concatenate([lo.ravel(), hi.ravel()])
                if mode == du.HARMONIC:
                    assert np.abs(got - c0).max() <= 2 * EPS * c0, (l, mode)
                else:
                    assert np.array_equal(got, np.full_like(got, c0 if mode == du.MEAN else 1.0 / c0)), (l, mode)


@pytest.mark.parametrize("name,n,div,dim", MESHES, ids=lambda v: str(v))
def test_weighted_fold_against_the_recipe(name, n, div, dim):
    m, H, levels = bc_util.setup(name, n, div, bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0], dim)
    for l, L in enumerate(levels):
        w = pu.unpack(positive(L.P * pu.face_size(n, dim), 20 + l), n, dim)
        bd = util.rand_vec(pu.num_bfaces(L) * L.nf, 30 + l)
        got, _ = du.boundary_rhs_weighted(L, w, bd)
        want = vc.boundary_rhs(L, w, bd)
        tol = 16 * EPS * dim * 2 * max(w[0].max(), w[1].max()) * np.abs(bd).max() / L.a["h"].min() ** 2
        err = np.abs(got - want).max()
        print(f"{name} level {l}: {err / tol:.3f} of the bound")
        assert err <= tol, l
        one = (np.ones_like(w[0]), np.ones_like(w[1]))
        # w = 1: the terms te_add_boundary_rhs folds, bit for bit
        assert np.array_equal(du.boundary_rhs_weighted(L, one, bd)[0], pu.level_boundary_rhs(L, bd)), l


def solve_error(div, n=8, dim=2):
    m, H, levels = util.setup("uniform", n, div, dim=dim)
    beta_fn, u_fn, F_fn = vc.manufactured2d()
    L, t = levels[0], H.tables(0)
    cc = vc.cell_centres(t, n, dim)
    rho = np.concatenate([(1.0 / beta_fn(*[cc[p, b] for b in range(dim)])).ravel() for p in range(L.P)])
    bc = vc.boundary_centres(L, t)
    rho_wall = 1.0 / beta_fn(*[bc[:, b] for b in range(dim)])
    beta = du.faces_from_cells(L, rho, du.RECIP_MEAN, rho_wall)
    betas = vc.restrict_all(levels, beta)
    exact = np.concatenate([u_fn(*[cc[p, b] for b in range(dim)]).ravel() for p in range(L.P)])
    F = np.concatenate([F_fn(*[cc[p, b] for b in range(dim)]).ravel() for p in range(L.P)])
    bd = u_fn(*[bc[:, b] for b in range(dim)])
    rhs, _ = du.boundary_rhs_weighted(L, beta, bd, F)
    x, its = vc.bicgstab(levels, betas, rhs, prolong_util.direct, tol=1e-12, coarse=32)
    return np.abs(x - exact).max()


def test_second_order_with_beta_from_cell_densities():
    errs = [solve_error(div) for div in (1, 2, 3)]
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print(f"max errors {errs}, ratios {ratios}")
    assert min(ratios) >= 3.5
