"""CPU: the numpy statement of the sub-patch coarse solve (tests/coefcoarse_util.py, the specification of te_gmg_set_coef_coarse) on
its own: the split is a relabelling of the one-patch level (split then merge is the identity, the operator on the split tree is the
operator on the patch, bit for bit), and the sub-cycle does what it is for (the iteration counts of DESIGN.md section 20).

Bounds (none of them comes from what the device gives):
  split / merge         equality: the values are moved, not computed
  operator              == 0: every term of (A_b u)[c] is formed from the same operands in the same order on both grids -- the ghost of a
                        face between two sub-patches is 2 ((m + v) / 2) - m on the split tree and v on the patch; the entries of
                        util.rand_vec and their sums are far from the range where the halving is inexact
  iteration counts      the table of DESIGN.md section 20 (sub_n = 4), +-0: the same composition on the same numbers"""
import functools

import numpy as np
import pytest

from tests import coefcoarse_util as cu, prolong_util, util, varcoef_util as vc

# (mesh, n, divides, dim): the hierarchies of the table; their coarsest levels are one patch of 8^3, 16^2, 16^2, 16^3, 32^2
SHAPES = [("uniform", 8, 1, 3), ("uniform", 16, 2, 2), ("2d2ref.bin", 16, 0, 2), ("uniform", 16, 1, 3), ("uniform", 32, 1, 2)]
# iterations to 1e-10, smooth beta / jump beta: sweeps 4, 16, 64, sub-cycle (cycles 1, coarse 4), sub-cycle (2, 8)
TABLE = {
    ("uniform", 8, 1, 3): ((9, 11), (7, 10), (7, 10), (8, 11), (7, 10)),
    ("uniform", 16, 2, 2): ((12, 14), (8, 11), (7, 10), (8, 11), (7, 10)),
    ("2d2ref.bin", 16, 0, 2): ((13, 14), (8, 11), (7, 11), (7, 12), (6, 10)),
    ("uniform", 16, 1, 3): ((15, 15), (9, 11), (7, 10), (10, 13), (8, 10)),
    ("uniform", 32, 1, 2): ((24, 22), (12, 12), (7, 9), (7, 10), (6, 9)),
}
COLUMNS = (("sweeps 4", None, 4), ("sweeps 16", None, 16), ("sweeps 64", None, 64), ("sub-cycle (1, 4)", 1, 4), ("sub-cycle (2, 8)", 2, 8))


@functools.lru_cache(maxsize=None)
def setup(name, n, div, dim):
    m, H, levels = util.setup(name, n, div, dim=dim)
    assert levels[-1].P == 1
    return H, levels


@pytest.mark.parametrize("name,n,div,dim", SHAPES, ids=lambda v: str(v))
def test_split_then_merge_is_the_identity(name, n, div, dim):
    H, levels = setup(name, n, div, dim)
    big = levels[-1]
    sub = cu.Sub(big, 4)
    v = util.rand_vec(big.size, 1)
    w = sub.split(v)
    assert w.shape == v.shape and np.array_equal(np.sort(w), np.sort(v))
    assert np.array_equal(sub.merge(w), v)
    assert np.array_equal(sub.split(sub.merge(w)), w)
    # the split beta: a shared face has equal copies, a face on the big patch's boundary is the big patch's
    beta = vc.random_beta_faces(big, 2)
    lo, hi = sub.split_faces(beta)
    A, shared = sub.levels[0], 0
    for q in range(A.P):
        for a in range(dim):
            ax = dim - 1 - a
            if A.a["nbr_kind"][q, 2 * a + 1] == 1:
                r = A.a["nbr"][q, 2 * a + 1, 0]
                assert np.array_equal(hi[q, a], np.take(lo[r, a], 0, axis=ax)), (q, a)
                shared += 1
            else:
                assert sub.origin[q][a] + 4 == n
    assert shared == dim * (n // 4 - 1) * (n // 4) ** (dim - 1)
    # merged back block by block, the lo blocks are the big patch's
    for a in range(dim):
        assert np.array_equal(sub.merge(lo[:, a].ravel()), beta[0][0, a].ravel())


@pytest.mark.parametrize("name,n,div,dim", SHAPES, ids=lambda v: str(v))
def test_the_operator_on_the_split_tree_is_the_operator_on_the_patch(name, n, div, dim):
    H, levels = setup(name, n, div, dim)
    big = levels[-1]
    beta = vc.random_beta_faces(big, 3)
    sigma = np.random.default_rng(4).uniform(0.0, 50.0, big.size)
    for s in [c for c in (4, 8) if cu.valid_sub_n(dim, n, c)]:
        sub = cu.Sub(big, s)
        sub.set_coefficient(beta, sigma)
        u = util.rand_vec(big.size, 5)
        diff = np.abs(vc.apply(sub.levels[0], sub.betas[0], sub.split(u)) - sub.split(vc.apply(big, beta, u))).max()
        print(f"A_b on the split tree against the patch, sub_n {s}: max difference {diff}")
        assert diff == 0, s
        diff = np.abs(vc.apply(sub.levels[0], sub.betas[0], sub.split(u), sub.sigmas[0]) - sub.split(vc.apply(big, beta, u, sigma))).max()
        print(f"A_b,sigma: max difference {diff}")
        assert diff == 0, s


def test_without_a_sub_cycle_the_composition_is_varcoef_utils():
    H, levels = setup("uniform", 8, 1, 3)
    betas = vc.restrict_all(levels, vc.random_beta_faces(levels[0], 6))
    f = util.rand_vec(levels[0].size, 7)
    zeros = [np.zeros(L.size) for L in levels]  # "no reaction term" as sigma = 0 on every level: the bits of sigmas=None
    for kw in (dict(coarse=4), dict(smoother=1, coarse=3, cycle_type=1)):
        assert np.array_equal(vc.cycle(levels, betas, f, prolong_util.direct, sigmas=zeros, sub=None, **kw), vc.cycle(levels, betas, f, prolong_util.direct, **kw)), kw


def test_sub_n_rule():
    assert [cu.auto_sub_n(3, n) for n in (4, 8, 16, 32)] == [None, 4, 8, 8]
    assert [cu.auto_sub_n(2, n) for n in (4, 6, 8, 10, 12, 16, 20, 64)] == [None, None, 4, None, 6, 4, 10, 4]
    assert cu.valid_sub_n(3, 32, 16) and not cu.valid_sub_n(3, 32, 32) and not cu.valid_sub_n(3, 24, 12) and not cu.valid_sub_n(2, 24, 8)


@pytest.mark.parametrize("beta_fn", [vc.smooth_beta, vc.jump_beta], ids=["smooth", "jump"])
@pytest.mark.parametrize("name,n,div,dim", SHAPES, ids=lambda v: str(v))
def test_iteration_table(name, n, div, dim, beta_fn):
    """BiCGStab to 1e-10, V(1,1) RB-GS, the direct interpolator, right-hand side rand_vec(size, 5), Dirichlet"""
    H, levels = setup(name, n, div, dim)
    betas = vc.restrict_all(levels, vc.beta_from(H.tables(0), n, dim, beta_fn))
    b = util.rand_vec(levels[0].size, 5)
    got = []
    for label, cycles, coarse in COLUMNS:
        sub = None if cycles is None else cu.make_sub(levels, betas, None, 4, cycles)
        x, its = vc.bicgstab(levels, betas, b, prolong_util.direct, sub=sub, tol=1e-10, coarse=coarse)
        assert np.linalg.norm(b - vc.apply(levels[0], betas[0], x)) <= 1e-9 * np.linalg.norm(b), label
        got.append(its)
    want = [col[beta_fn is vc.jump_beta] for col in TABLE[(name, n, div, dim)]]
    print(f"{name} n {n} div {div} {dim}d {beta_fn.__name__}: {dict(zip([c[0] for c in COLUMNS], got))}")
    assert got == want
