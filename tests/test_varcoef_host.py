"""CPU: the numpy statement of the variable-coefficient operator (tests/varcoef_util.py, the specification of
te_gmg_set_coefficient's path) on its own: with beta = 1 it is the oracle's operator and sweeps, the face restriction reproduces
linear fields, the discretisation is second order, and the composed cycle preconditions BiCGStab through smooth and jumping
coefficients.

Bounds (none of them comes from what the device gives):
  apply, beta = 1       util.op_tol: a few ulps of sum |coef| |u|
  rbgs, beta = 1        4 eps max|u| (u the input iterate) per sweep on the oracle's own input (the same sums in another association)
  jacobi, beta = 1      op_tol scaled by omega / d_min, d_min >= rh2_min (one face of the smallest diagonal), plus 4 eps max|u|
  restrict_faces        a linear field's face averages ARE its values at the coarse face centres: 16 eps max|field|
  order                 consecutive max-error ratios >= 3.5 (second order: 4 in the limit)
  solve                 <= 15 iterations to 1e-10: a cap the composition stays under on these inputs, not a property of a kernel"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import bc_util, projection_util as pu, prolong_util, util, varcoef_util as vc
from tests.varcoef_util import SOLVES

MESHES = [("uniform", 4, 2, 3), ("2refine.bin", 4, 0, 3), ("2d2ref.bin", 8, 1, 2), ("uniform", 8, 2, 2)]


def ones(L):
    return np.ones((L.P, L.dim) + (L.n,) * L.dim), np.ones((L.P, L.dim) + (L.n,) * (L.dim - 1))


def setup(name, n, div, dim, mask):
    if mask == 0:
        return util.setup(name, n, div, dim=dim)
    if mask == (1 << 2 * dim) - 1:
        return util.setup(name, n, div, neumann=True, dim=dim)
    return bc_util.setup(name, n, div, mask, dim)


@pytest.mark.parametrize("mask_kind", ["dirichlet", "neumann", "mixed"])
@pytest.mark.parametrize("name,n,div,dim", MESHES, ids=lambda v: str(v))
def test_beta_one_is_the_oracle(name, n, div, dim, mask_kind):
    mask = {"dirichlet": 0, "neumann": (1 << 2 * dim) - 1, "mixed": bc_util.CHANNEL if dim == 3 else bc_util.MASKS2[0]}[mask_kind]
    m, H, levels = setup(name, n, div, dim, mask)
    for l, L in enumerate(levels):
        u, f = util.rand_vec(L.size, 10 + l), util.rand_vec(L.size, 20 + l)
        one = ones(L)
        err, tol = np.abs(vc.apply(L, one, u) - orc.apply(L, u)).max(), util.op_tol(L, u)
        print(f"{name} {mask_kind} level {l}: apply {err / tol:.3f} of op_tol")
        assert err <= tol, l
        err = np.abs(vc.rbgs(L, one, f, u) - orc.patch_rbgs(L, f, u)).max()
        big = np.abs(u).max()
        print(f"{name} {mask_kind} level {l}: rbgs {err:.3e} (4 eps max|u| = {4 * util.EPS * big:.3e})")
        assert err <= 4 * util.EPS * big, l
        omega = 6.0 / 7.0
        rh2min = (1.0 / L.a["h"].max() ** 2)
        tolj = omega * (util.op_tol(L, u) + 4 * util.EPS * np.abs(f).max()) / rh2min + 4 * util.EPS * np.abs(u).max()
        err = np.abs(vc.jacobi(L, one, f, u, omega) - orc.jacobi(L, f, u, omega)).max()
        print(f"{name} {mask_kind} level {l}: jacobi {err / tolj:.3f} of its bound")
        assert err <= tolj, l


@pytest.mark.parametrize("name,n,div,dim", MESHES + [("multi_refine.bin", 4, 0, 3)], ids=lambda v: str(v))
def test_face_restriction_reproduces_linear_fields(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    assert len(levels) >= 2
    coef = [0.7, -1.3, 2.1][:dim]
    fn = lambda *x: 3.0 + sum(c * xi for c, xi in zip(coef, x))
    copies = 0
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        fine, want = vc.beta_from(H.tables(l), n, dim, fn), vc.beta_from(H.tables(l + 1), n, dim, fn)
        got = vc.restrict_faces(F, C, fine)
        err = max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())
        print(f"{name} level {l}: {err:.3e}")
        assert err <= 16 * util.EPS * 8.0, l
        for pf in range(F.P):
            if F.a["orth_on_parent"][pf] < 0:  # copy-through: bit for bit
                copies += 1
                pc = F.a["parent"][pf]
                assert np.array_equal(got[0][pc], fine[0][pf]) and np.array_equal(got[1][pc], fine[1][pf])
    if name.endswith(".bin"):
        assert copies > 0


def solve_error(name, div, n=8, dim=2):
    m, H, levels = util.setup(name, n, div, dim=dim)
    betas, rhs, exact = vc.manufactured_problem(H, levels, n, dim, *vc.manufactured2d())
    x, its = vc.bicgstab(levels, betas, rhs, prolong_util.direct, tol=1e-12, coarse=32)
    return np.abs(x - exact).max()


@pytest.mark.parametrize("name", ["uniform", "2d2ref.bin"])
def test_second_order(name):
    errs = [solve_error(name, div) for div in (1, 2, 3)]
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print(f"{name}: max errors {errs}, ratios {ratios}")
    assert min(ratios) >= 3.5


@pytest.mark.parametrize("interp", ["direct", "linear"])
@pytest.mark.parametrize("beta_fn", [vc.smooth_beta, vc.jump_beta], ids=["smooth", "jump"])
@pytest.mark.parametrize("name,n,div,dim", SOLVES, ids=lambda v: str(v))
def test_cycle_preconditions_bicgstab(name, n, div, dim, beta_fn, interp):
    m, H, levels = util.setup(name, n, div, dim=dim)
    betas = vc.restrict_all(levels, vc.beta_from(H.tables(0), n, dim, beta_fn))
    b = util.rand_vec(levels[0].size, 5)
    prolong = prolong_util.direct if interp == "direct" else prolong_util.prolong_linear_add
    x, its = vc.bicgstab(levels, betas, b, prolong, tol=1e-10, max_it=40, coarse=32 if dim == 2 else 16)
    rel = np.linalg.norm(b - vc.apply(levels[0], betas[0], x)) / np.linalg.norm(b)
    print(f"{name} {dim}d {beta_fn.__name__} {interp}: {its} iterations, true relative residual {rel:.2e}")
    assert its <= 15 and rel <= 1e-9
