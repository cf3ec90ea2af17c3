"""CPU: the numpy statement of the linear interpolator (tests/prolong_util.py, the specification of TE_INTERP_LINEAR) on its own:
constants and affine functions are reproduced, the Python composition of a cycle is the oracle's cycle, and the statement buys
what it was added for -- a convergence factor that does not grow with the depth of the hierarchy, and fewer BiCGStab iterations."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import prolong_util as pu, util

# (mesh, n, divides, dim)
ONES = [("2refine.bin", 4, 0, 3), ("2refine.bin", 8, 0, 3), ("multi_refine.bin", 4, 0, 3), ("2d2ref.bin", 4, 0, 2), ("uniform", 4, 2, 3),
        ("uniform", 4, 2, 2)]


@pytest.mark.parametrize("name,n,div,dim", ONES, ids=lambda v: str(v))
def test_constant_is_reproduced_on_neumann_hierarchies(name, n, div, dim):
    """P(1) = 1 on every level pair, coarse/fine faces, edges and corners included (an all-Neumann hierarchy: no Dirichlet ghost)"""
    m, H, levels = util.setup(name, n, div, neumann=True, dim=dim)
    assert len(levels) >= 2
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        got = pu.prolong_linear_add(F, C, np.ones(C.size), np.zeros(F.size))
        err = np.abs(got - 1.0).max()
        print(f"{name} n={n} level {l}: |P(1) - 1| = {err:.3e}")
        assert err <= 64 * util.EPS, l


def centres(t, n, dim):
    """cell centres of a level from the hierarchy's tables -> [P * n^dim, dim], x fastest"""
    idx = np.indices((n,) * dim)[::-1].reshape(dim, -1).T  # column a = index along axis a, x fastest
    h = t["lengths"] / n
    return (t["starts"][:, None, :] + (idx[None, :, :] + 0.5) * h[:, None, :]).reshape(-1, dim)


@pytest.mark.parametrize("n,div,dim", [(4, 2, 3), (8, 1, 3), (4, 2, 2), (8, 2, 2)])
def test_affine_is_reproduced_away_from_physical_ghosts(n, div, dim):
    m, H, levels = util.setup("uniform", n, div, dim=dim)
    coef, off = np.array([0.7, -1.3, 2.1])[:dim], 0.4
    for l in range(len(levels) - 1):
        F, C = levels[l], levels[l + 1]
        tf, tc = H.tables(l), H.tables(l + 1)
        xf, xc = centres(tf, n, dim), centres(tc, n, dim)
        got = pu.prolong_linear_add(F, C, xc @ coef + off, np.zeros(F.size))
        lo, hi = tf["starts"].min(axis=0), (tf["starts"] + tf["lengths"]).max(axis=0)
        hf = (tf["lengths"] / n).max(axis=0)
        inner = np.all((xf > lo + hf) & (xf < hi - hf), axis=1)  # the first and last fine layer read a Dirichlet ghost
        assert inner.sum() > 0
        err = np.abs(got - (xf @ coef + off))[inner].max()
        print(f"n={n} div={div} {dim}d level {l}: affine error {err:.3e} on {inner.sum()} of {inner.size} cells")
        assert err <= 1e-13, l


@pytest.mark.parametrize("smoother,cycle_type,pre", [(2, 0, 1), (2, 1, 1), (0, 0, 1), (1, 0, 2)])
@pytest.mark.parametrize("name,n,div,dim", [("uniform", 4, 2, 3), ("2refine.bin", 4, 0, 3), ("2d2ref.bin", 4, 0, 2)], ids=lambda v: str(v))
def test_composition_is_the_oracle_cycle(name, n, div, dim, smoother, cycle_type, pre):
    m, H, levels = util.setup(name, n, div, dim=dim)
    f = util.rand_vec(levels[0].size, 3)
    want = orc.cycle(levels, orc.cycle_opts(pre=pre, post=pre, smoother=smoother, cycle_type=cycle_type), f)
    got = pu.cycle(levels, f, pu.direct, smoother=smoother, pre=pre, post=pre, cycle_type=cycle_type)
    assert np.abs(got - want).max() == 0.0


# (n, 8th-cycle reduction: linear at most / DrctIntp at least, BiCGStab iterations: linear at most / DrctIntp at least)
@pytest.mark.parametrize("n,red_lin,red_dir,its_lin,its_dir", [(8, 0.32, 0.45, 8, 10), (4, 0.32, 0.45, 8, 9)])
def test_linear_prolongation_converges_faster(n, red_lin, red_dir, its_lin, its_dir):
    """uniform, 2 divides, Dirichlet, V(1,1) with RB-GS, f ~ U(-1, 1) from default_rng(0)"""
    m, H, levels = util.setup("uniform", n, 2)
    f = util.rand_vec(levels[0].size, 0)
    rl, rd = pu.reductions(levels, f, pu.prolong_linear_add)[-1], pu.reductions(levels, f, pu.direct)[-1]
    il, idr = pu.bicgstab(levels, f, pu.prolong_linear_add)[1], pu.bicgstab(levels, f, pu.direct)[1]
    print(f"n={n}: 8th-cycle reduction linear {rl:.3f} DrctIntp {rd:.3f}; BiCGStab iterations linear {il} DrctIntp {idr}")
    assert rl <= red_lin and rd >= red_dir
    assert il <= its_lin and idr >= its_dir
