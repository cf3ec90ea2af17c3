"""The one numpy statement of the multigrid cycle (GMG/Cycle.h:56-126 with VCycle.h / WCycle.h) and of BiCGStab (BiCGStab.h:45-106)
behind the specification modules: tests/prolong_util.py (the Laplacian, the oracle's pieces) and tests/varcoef_util.py (A_b and
A_b - sigma, with tests/coefcoarse_util.py's sub-patch coarse solve) compose theirs from these by handing in closures. The driver
knows no smoother, coefficient or sigma: the order of the floating-point statements below is the specification, and
tests/test_prolong_host.py::test_composition_is_the_oracle_cycle holds it to the oracle's compiled cycle at 0.0.

    visit      the cycle from level l on, u CARRIED into the level; the coarser levels start from zero
    cycle      visit from level 0 on a zero iterate
    bicgstab   right-preconditioned, x0 = 0 -> (x, iterations)"""
import numpy as np

from oracle import oracle as orc


def visit(levels, l, f, u, apply, smooth, prolong, coarsest=None, pre=1, post=1, coarse=1, mid=1, cycle_type=0):
    """apply(l, u) and smooth(l, f, u) are the caller's operator and sweep on level l, prolong(F, C, e, u) = u + P e; the last level
    runs `coarse` sweeps, or coarsest(f, u) where one is given. cycle_type: 0 V, 1 W (`mid` sweeps between the two descents)."""
    L = levels[l]
    if l == len(levels) - 1:
        if coarsest is not None:
            return coarsest(f, u)
        for _ in range(coarse):
            u = smooth(l, f, u)
        return u

    def descend(u):
        r = -1 * apply(l, u) + f
        cf = orc.restrict(L, levels[l + 1], r)
        cu = visit(levels, l + 1, cf, np.zeros(levels[l + 1].size), apply, smooth, prolong, coarsest, pre, post, coarse, mid, cycle_type)
        return prolong(L, levels[l + 1], cu, u)

    for _ in range(pre):
        u = smooth(l, f, u)
    u = descend(u)
    if cycle_type == 1:
        for _ in range(mid):
            u = smooth(l, f, u)
        u = descend(u)
    for _ in range(post):
        u = smooth(l, f, u)
    return u


def cycle(levels, f, apply, smooth, prolong, coarsest=None, **kw):
    return visit(levels, 0, np.ascontiguousarray(f, np.float64), np.zeros(levels[0].size), apply, smooth, prolong, coarsest, **kw)


def bicgstab(A, M, b, max_it=100, tol=1e-12):
    """A the operator, M the preconditioner (one cycle), both callables on a vector -> (x, iterations)"""
    x = np.zeros(len(b))
    resid = -1 * A(x) + b
    r0 = np.linalg.norm(resid)
    rhat, p = resid.copy(), resid.copy()
    rho = rhat @ resid
    its = 0
    while np.linalg.norm(resid) / r0 > tol and its < max_it:
        mp = M(p)
        ap = A(mp)
        alpha = rho / (rhat @ ap)
        s = resid + ap * -alpha
        ms = M(s)
        as_ = A(ms)
        omega = (as_ @ s) / (as_ @ as_)
        x = x + mp * alpha + ms * omega
        resid = resid + ap * -alpha + as_ * -omega
        rho_new = resid @ rhat
        beta = rho_new * alpha / (rho * omega)
        p = beta * (p + ap * -omega) + resid
        its += 1
        rho = rho_new
    return x, its
