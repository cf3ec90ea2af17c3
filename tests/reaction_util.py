"""The numpy statement of the reaction term: A_bs u = div(beta grad u) - sigma u (include/te_hip.h te_gmg_set_reaction, DESIGN.md
section 19), the specification the device kernels are held to. Built on tests/varcoef_util.py (A_b, its diagonals and ghosts) and the
oracle (restriction, interface interpolation) by import.

sigma of a level is a cell vector in the level's layout (L.size doubles), every entry >= 0; beta as in varcoef_util.

    apply      (A_b u)[c] - sigma_c u_c: A_b exactly as varcoef_util.apply, then one multiplication and one subtraction
    rbgs       u_c <- (o - f_c) / (d + sigma_c), o and d as in varcoef_util.rbgs; colour order and frozen ghosts unchanged
    jacobi     u + omega (f - A_bs u) / (-(d_J + sigma_c))
    restrict_all     level l + 1's sigma = orc.restrict (te_restrict's average) of level l's; copy-through patches bit for bit
    cycle / bicgstab varcoef_util's, composed from these

With sigma = 0 every function returns varcoef_util's bits (tests/test_reaction_host.py)."""
import numpy as np

from oracle import oracle as orc
from tests import varcoef_util as vc


def _cells(L, v):
    return np.asarray(v, np.float64).reshape((L.P,) + (L.n,) * L.dim)


def apply(L, beta, sigma, u):
    u = np.asarray(u, np.float64)
    return vc.apply(L, beta, u) - np.asarray(sigma, np.float64) * u


def jacobi(L, beta, sigma, f, u, omega):
    n, D = L.n, L.dim
    _, _, adj = vc._side_tables(L)
    r = _cells(L, np.asarray(f) - apply(L, beta, sigma, u))
    S = _cells(L, sigma)
    out = _cells(L, u).copy()
    for p in range(L.P):
        d = np.zeros((n,) * D)
        for a in range(D):
            blo, bhi = vc._beta_sides(L, beta, p, a)
            w_lo, w_hi = vc._face_weights(L, p, a, 1.0 + adj[p, 2 * a], 1.0 + adj[p, 2 * a + 1])
            rh2 = 1.0 / L.a["h"][p, a] ** 2
            d += blo * w_lo * rh2
            d += bhi * w_hi * rh2
        d = d + S[p]
        out[p] += omega * r[p] / (-d)
    return out.ravel()


def rbgs(L, beta, sigma, f, u):
    n, D = L.n, L.dim
    isdir, isneu, _ = vc._side_tables(L)
    U, F, S = _cells(L, u), _cells(L, f), _cells(L, sigma)
    gam, ii = orc.interp(L, np.asarray(u, np.float64)), L.iface_index()
    out = U.copy()
    idx = np.indices((n,) * D).sum(axis=0)
    for p in range(L.P):
        d = np.zeros((n,) * D)
        ghosts, bs, rh2s = [], [], []
        for a in range(D):
            ax = vc._ax(L, a)
            blo, bhi = vc._beta_sides(L, beta, p, a)
            kap = [2.0 if isdir[p, 2 * a + k] else (0.0 if isneu[p, 2 * a + k] else 1.0) for k in (0, 1)]
            w_lo, w_hi = vc._face_weights(L, p, a, kap[0], kap[1])
            rh2 = 1.0 / L.a["h"][p, a] ** 2
            d += blo * w_lo * rh2
            d += bhi * w_hi * rh2
            gh = []
            for k in (0, 1):
                s = 2 * a + k
                if L.a["nbr_kind"][p, s] == 0:
                    gh.append(np.zeros((n,) * (D - 1)))  # physical faces contribute nothing to o
                else:
                    m = np.take(U[p], n - 1 if k else 0, axis=ax)
                    gh.append(2 * gam[ii[p, s] * L.nf:(ii[p, s] + 1) * L.nf].reshape((n,) * (D - 1)) - m)  # frozen at the old iterate
            ghosts.append(gh)
            bs.append((blo, bhi))
            rh2s.append(rh2)
        d = d + S[p]  # the one change: the diagonal of A_bs is -(d + sigma)
        cur = U[p].copy()
        for colour in (0, 1):
            o = np.zeros((n,) * D)
            for a in range(D):
                ax = vc._ax(L, a)
                ext = np.concatenate([np.expand_dims(ghosts[a][0], ax), cur, np.expand_dims(ghosts[a][1], ax)], axis=ax)
                o += bs[a][0] * np.take(ext, np.arange(0, n), axis=ax) * rh2s[a]
                o += bs[a][1] * np.take(ext, np.arange(2, n + 2), axis=ax) * rh2s[a]
            new = (o - F[p]) / d
            mask = (idx & 1) == colour
            cur[mask] = new[mask]
        out[p] = cur
    return out.ravel()


def restrict_all(levels, sigma0):
    sigmas = [np.ascontiguousarray(sigma0, np.float64)]
    for l in range(len(levels) - 1):
        sigmas.append(orc.restrict(levels[l], levels[l + 1], sigmas[-1]))
    return sigmas


def cycle(levels, betas, sigmas, f, prolong, smoother=2, pre=1, post=1, coarse=1, mid=1, cycle_type=0, omega=6.0 / 7.0):
    """varcoef_util.cycle with A_bs and its sweeps (smoother: 1 Jacobi, 2 patch-local RB-GS)"""
    nl = len(levels)

    def smooth(l, f, u):
        if smoother == 1:
            return jacobi(levels[l], betas[l], sigmas[l], f, u, omega)
        return rbgs(levels[l], betas[l], sigmas[l], f, u)

    def visit(l, f, u):
        L = levels[l]
        if l == nl - 1:
            for _ in range(coarse):
                u = smooth(l, f, u)
            return u

        def descend(u):
            r = -1 * apply(L, betas[l], sigmas[l], u) + f
            cf = orc.restrict(L, levels[l + 1], r)
            cu = visit(l + 1, cf, np.zeros(levels[l + 1].size))
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

    return visit(0, np.ascontiguousarray(f, np.float64), np.zeros(levels[0].size))


def bicgstab(levels, betas, sigmas, b, prolong, max_it=100, tol=1e-12, **kw):
    """varcoef_util.bicgstab with A_bs, right-preconditioned by the composed cycle -> (x, iterations). No mean shift anywhere."""
    L = levels[0]
    A = lambda v: apply(L, betas[0], sigmas[0], v)
    M = lambda v: cycle(levels, betas, sigmas, v, prolong, **kw)
    x = np.zeros(L.size)
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


def sigma_from(t, n, dim, fn):
    """fn(x, y[, z]) at the cell centres of level tables t -> a cell vector"""
    cc = vc.cell_centres(t, n, dim)
    return np.concatenate([(fn(*[cc[p, b] for b in range(dim)]) + 0.0 * cc[p, 0]).ravel() for p in range(len(cc))])


# ---- the problems of the tests
def manufactured2d():
    """beta = exp(x + y), u = sin(2x + 0.3) sin(3y + 0.1), sigma = 1 + x^2 + y^2, F = div(beta grad u) - sigma u"""
    beta, u, F0 = vc.manufactured2d()
    sigma = lambda x, y: 1.0 + x * x + y * y
    F = lambda x, y: F0(x, y) - sigma(x, y) * u(x, y)
    return beta, sigma, u, F


def manufactured3d():
    """beta = exp(x + y + z), u = sin(2x + 0.3) sin(3y + 0.1) sin(1.5z + 0.2), sigma = 1 + x^2 + y^2 + z^2"""
    beta = lambda x, y, z: np.exp(x + y + z)
    sx, sy, sz = (lambda x: np.sin(2 * x + 0.3)), (lambda y: np.sin(3 * y + 0.1)), (lambda z: np.sin(1.5 * z + 0.2))
    cx, cy, cz = (lambda x: np.cos(2 * x + 0.3)), (lambda y: np.cos(3 * y + 0.1)), (lambda z: np.cos(1.5 * z + 0.2))
    u = lambda x, y, z: sx(x) * sy(y) * sz(z)
    sigma = lambda x, y, z: 1.0 + x * x + y * y + z * z
    F = lambda x, y, z: np.exp(x + y + z) * (-(4 + 9 + 2.25) * u(x, y, z) + 2 * cx(x) * sy(y) * sz(z) + 3 * sx(x) * cy(y) * sz(z)
                                             + 1.5 * sx(x) * sy(y) * cz(z)) - sigma(x, y, z) * u(x, y, z)
    return beta, sigma, u, F


def manufactured_problem(H, levels, n, dim, beta_fn, sigma_fn, u_fn, F_fn):
    """-> (betas, sigmas per level, right-hand side with the boundary terms of section 18's recipe (1) -- unchanged, sigma multiplies no
    ghost --, exact solution at the cell centres)"""
    betas, rhs, exact = vc.manufactured_problem(H, levels, n, dim, beta_fn, u_fn, F_fn)
    return betas, restrict_all(levels, sigma_from(H.tables(0), n, dim, sigma_fn)), rhs, exact
