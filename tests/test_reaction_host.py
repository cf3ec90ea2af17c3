"""CPU: the numpy statement of the reaction term A_bs u = div(beta grad u) - sigma u (tests/varcoef_util.py with `sigma=`, and
tests/reaction_util.py: the specification of te_gmg_set_reaction's path) on its own: with sigma = 0 it is the statement without sigma
(`sigma=None`: the `- sigma u` and `d + sigma` statements are not executed) bit for bit, sigma goes down the levels by the
oracle's restriction, the discretisation stays second order, a larger diagonal does not cost iterations, and the all-Neumann problem
is nonsingular.

Bounds (none of them comes from what the device gives):
  sigma = 0             bit for bit: only `- 0 * u` and `d + 0` enter
  restriction           equality with orc.restrict (it IS that function, level by level); copy-through patches bit for bit
  order                 each max-error ratio within 0.15 of the sigma = 0 ratio of the same run: the spread between the uniform and the
                        refined sigma = 0 figures (3.996 / 3.999 against 3.87 / 3.92)
  convergence           iterations to 1e-10 <= the sigma = 0 count of the same case: a larger diagonal can only help a diagonally
                        scaled smoother
  all-Neumann           max|f - A_bs x| <= 1e-10 max|f| with no mean shift anywhere in the composition"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import bc_util, prolong_util, reaction_util as ru, util, varcoef_util as vc
from tests.varcoef_util import SOLVES

ZERO_MESHES = [("uniform", 8, 2, 2), ("2d2ref.bin", 8, 1, 2), ("uniform", 4, 1, 3), ("2refine.bin", 4, 0, 3)]


@pytest.mark.parametrize("mask_kind", ["dirichlet", "mixed"])
@pytest.mark.parametrize("name,n,div,dim", ZERO_MESHES, ids=lambda v: str(v))
def test_sigma_zero_changes_nothing(name, n, div, dim, mask_kind):
    mask = 0 if mask_kind == "dirichlet" else (bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0])
    m, H, levels = bc_util.setup(name, n, div, mask, dim)
    betas = vc.restrict_all(levels, vc.random_beta_faces(levels[0], 7))
    zeros = [np.zeros(L.size) for L in levels]
    omega = 6.0 / 7.0
    for l, L in enumerate(levels):
        u, f = util.rand_vec(L.size, 10 + l), util.rand_vec(L.size, 20 + l)
        assert np.array_equal(vc.apply(L, betas[l], u, zeros[l]), vc.apply(L, betas[l], u)), l
        assert np.array_equal(vc.rbgs(L, betas[l], f, u, zeros[l]), vc.rbgs(L, betas[l], f, u)), l
        assert np.array_equal(vc.jacobi(L, betas[l], f, u, omega, zeros[l]), vc.jacobi(L, betas[l], f, u, omega)), l
    f = util.rand_vec(levels[0].size, 30)
    for kw in (dict(smoother=2, coarse=4), dict(smoother=1, coarse=4, cycle_type=1)):
        got = vc.cycle(levels, betas, f, prolong_util.direct, sigmas=zeros, **kw)
        assert np.array_equal(got, vc.cycle(levels, betas, f, prolong_util.direct, **kw)), kw


@pytest.mark.parametrize("name,n,div,dim", ZERO_MESHES + [("multi_refine.bin", 4, 0, 3)], ids=lambda v: str(v))
def test_restriction(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    assert len(levels) >= 2
    sigmas = ru.restrict_all(levels, np.random.default_rng(11).uniform(0.0, 50.0, levels[0].size))
    assert len(sigmas) == len(levels)
    copies = 0
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        assert sigmas[l + 1].shape == (C.size,)
        assert np.array_equal(sigmas[l + 1], orc.restrict(F, C, sigmas[l])), l
        assert sigmas[l + 1].min() >= 0.0 and sigmas[l + 1].max() <= 50.0  # an average
        fine, coarse = sigmas[l].reshape(F.P, -1), sigmas[l + 1].reshape(C.P, -1)
        for pf in range(F.P):
            if F.a["orth_on_parent"][pf] < 0:  # copy-through: bit for bit
                copies += 1
                assert np.array_equal(coarse[F.a["parent"][pf]], fine[pf]), (l, pf)
    if name.endswith(".bin"):
        assert copies > 0


def solve_errors(name, div, n=8, dim=2):
    """max errors of the manufactured problem with sigma and with sigma = 0, the same mesh"""
    m, H, levels = util.setup(name, n, div, dim=dim)
    betas, sigmas, rhs, exact = ru.manufactured_problem(H, levels, n, dim, *ru.manufactured2d())
    x, _ = vc.bicgstab(levels, betas, rhs, prolong_util.direct, tol=1e-12, sigmas=sigmas, coarse=32)
    betas0, rhs0, exact0 = vc.manufactured_problem(H, levels, n, dim, *vc.manufactured2d())
    x0, _ = vc.bicgstab(levels, betas0, rhs0, prolong_util.direct, tol=1e-12, coarse=32)
    return np.abs(x - exact).max(), np.abs(x0 - exact0).max()


@pytest.mark.parametrize("name", ["uniform", "2d2ref.bin"])
def test_second_order(name):
    errs = [solve_errors(name, div) for div in (1, 2, 3)]
    ratios = [errs[i][0] / errs[i + 1][0] for i in range(2)]
    ratios0 = [errs[i][1] / errs[i + 1][1] for i in range(2)]
    print(f"{name}: max errors (sigma, sigma = 0) {errs}, ratios {ratios}, with sigma = 0 {ratios0}")
    for r, r0 in zip(ratios, ratios0):
        assert abs(r - r0) <= 0.15


def sigma_cases(H, n, dim, beta_fn):
    """sigma = 100, and sigma = rho / dt with rho = 1 / beta at the cell centres, dt = 1e-3"""
    return {"hundred": ru.sigma_from(H.tables(0), n, dim, lambda *x: 100.0), "rho_over_dt": ru.sigma_from(H.tables(0), n, dim, lambda *x: 1.0 / beta_fn(*x) / 1e-3)}


@pytest.mark.parametrize("beta_fn", [vc.smooth_beta, vc.jump_beta], ids=["smooth", "jump"])
@pytest.mark.parametrize("name,n,div,dim", SOLVES, ids=lambda v: str(v))
def test_a_larger_diagonal_does_not_cost_iterations(name, n, div, dim, beta_fn):
    m, H, levels = util.setup(name, n, div, dim=dim)
    betas = vc.restrict_all(levels, vc.beta_from(H.tables(0), n, dim, beta_fn))
    b = util.rand_vec(levels[0].size, 5)
    coarse = 32 if dim == 2 else 16
    _, its0 = vc.bicgstab(levels, betas, b, prolong_util.direct, tol=1e-10, max_it=40, coarse=coarse)
    for kind, sigma0 in sigma_cases(H, n, dim, beta_fn).items():
        sigmas = ru.restrict_all(levels, sigma0)
        x, its = vc.bicgstab(levels, betas, b, prolong_util.direct, tol=1e-10, max_it=40, sigmas=sigmas, coarse=coarse)
        rel = np.linalg.norm(b - vc.apply(levels[0], betas[0], x, sigmas[0])) / np.linalg.norm(b)
        print(f"{name} {dim}d {beta_fn.__name__} {kind}: {its} iterations ({its0} with sigma = 0), true relative residual {rel:.2e}")
        assert rel <= 1e-9
        assert its <= its0, kind


@pytest.mark.parametrize("name,n,div,dim", SOLVES, ids=lambda v: str(v))
def test_all_neumann_with_sigma_is_nonsingular(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, neumann=True, dim=dim)
    betas = vc.restrict_all(levels, vc.beta_from(H.tables(0), n, dim, vc.smooth_beta))
    sigmas = ru.restrict_all(levels, ru.sigma_from(H.tables(0), n, dim, lambda *x: 1.0 + sum(xi * xi for xi in x)))
    f = util.rand_vec(levels[0].size, 6) + 0.5  # (its mean is not zero: the pure Neumann problem would have no solution)
    x, its = vc.bicgstab(levels, betas, f, prolong_util.direct, tol=1e-12, max_it=40, sigmas=sigmas, coarse=32 if dim == 2 else 16)
    r = f - vc.apply(levels[0], betas[0], x, sigmas[0])
    print(f"{name} {dim}d: {its} iterations, max|f - A x| / max|f| = {np.abs(r).max() / np.abs(f).max():.2e}, mean(x) = {x.mean():.3e}")
    assert its < 40
    assert np.linalg.norm(r) <= 1e-10 * np.linalg.norm(f)
    assert np.abs(r).max() <= 1e-10 * np.abs(f).max()
