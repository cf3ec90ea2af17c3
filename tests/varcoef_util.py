"""The numpy statement of the variable-coefficient operator A_b u = div(beta grad u) (include/te_hip.h): the
specification the device kernels are held to, composed from the pieces the other features are held to -- projection_util's MAC
gradient / divergence, prolong_util's interpolators, the oracle's restriction and interface interpolation.

beta of a level is a pair (lo, hi) in projection_util's layout: lo[p, a] has the shape of a patch (numpy index order z, y, x): beta
on the lower a-face of each cell; hi[p, a] has the shape of a face: beta on the patch's upper a-face.

    apply      div(beta (.) grad u), the ghosts of grad those of te_apply (2 gamma - m, -m Dirichlet, +m Neumann)
    rbgs       patch-local, red = (x + y + z) even first, ghosts of faces with a neighbour frozen at the old iterate;
               u_c <- (o - f_c) / d, o = sum_s b_s v_s rh2_a (physical faces 0), d = sum_s b_s kappa_s rh2_a, kappa 1 / 2 (D) / 0 (N)
    jacobi     u + omega (f - A_b u) / (-d_J), d_J = sum_s b_s (1 + adj_s) rh2_a, adj = orc_jacobi's adjustment per side
    restrict_faces   the face average of the 2^(dim-1) fine faces that cover a coarse face; copy-through patches bit for bit
    cycle / bicgstab GMG/Cycle.h:56-126 and BiCGStab.h:45-106 composed from these, no exact coarse solve"""
import numpy as np

from oracle import oracle as orc
from tests import projection_util as pu


def _ax(L, a):
    return L.dim - 1 - a  # numpy axis of coordinate a inside a patch


def apply(L, beta, u):
    lo, hi = pu.level_grad(L, u)
    return pu.level_div(L, lo * beta[0], hi * beta[1])


def _side_tables(L):
    """per (patch, side): physical Dirichlet / Neumann flags and the Jacobi adjustment"""
    kind, neu = L.a["nbr_kind"], L.a["neumann"]
    s = np.arange(2 * L.dim)
    phys = kind == 0
    isneu = phys & (((neu[:, None] >> s[None, :]) & 1) == 1)
    isdir = phys & ~isneu
    adj = np.zeros(kind.shape)
    adj[isdir] = 1.0
    adj[isneu] = -1.0
    adj[kind == 2] = -5.0 / 6.0 if L.dim == 3 else -2.0 / 3.0
    adj[kind == 3] = 1.0 / 3.0
    return isdir, isneu, adj


def _beta_sides(L, beta, p, a):
    """beta on the lower and on the upper a-face of every cell of patch p"""
    ax = _ax(L, a)
    full = np.concatenate([beta[0][p, a], np.expand_dims(beta[1][p, a], ax)], axis=ax)
    n = L.n
    return np.take(full, np.arange(n), axis=ax), np.take(full, np.arange(1, n + 1), axis=ax)


def _face_weights(L, p, a, low, high, inner=1.0):
    """an array of the patch's shape: `inner` everywhere, `low` on the cells of the lower a-face, `high` on those of the upper one
    -- for the LOWER side of the cells (w_lo) and for the UPPER side (w_hi)"""
    shape, ax = (L.n,) * L.dim, _ax(L, a)
    w_lo, w_hi = np.full(shape, inner), np.full(shape, inner)
    sl = [slice(None)] * L.dim
    sl[ax] = 0
    w_lo[tuple(sl)] = low
    sl[ax] = L.n - 1
    w_hi[tuple(sl)] = high
    return w_lo, w_hi


def jacobi(L, beta, f, u, omega):
    n, D = L.n, L.dim
    _, _, adj = _side_tables(L)
    r = (np.asarray(f) - apply(L, beta, u)).reshape((L.P,) + (n,) * D)
    out = np.asarray(u, np.float64).reshape((L.P,) + (n,) * D).copy()
    for p in range(L.P):
        d = np.zeros((n,) * D)
        for a in range(D):
            blo, bhi = _beta_sides(L, beta, p, a)
            w_lo, w_hi = _face_weights(L, p, a, 1.0 + adj[p, 2 * a], 1.0 + adj[p, 2 * a + 1])
            rh2 = 1.0 / L.a["h"][p, a] ** 2
            d += blo * w_lo * rh2
            d += bhi * w_hi * rh2
        out[p] += omega * r[p] / (-d)
    return out.ravel()


def rbgs(L, beta, f, u):
    n, D = L.n, L.dim
    isdir, isneu, _ = _side_tables(L)
    U = np.asarray(u, np.float64).reshape((L.P,) + (n,) * D)
    F = np.asarray(f, np.float64).reshape((L.P,) + (n,) * D)
    gam, ii = orc.interp(L, np.asarray(u, np.float64)), L.iface_index()
    out = U.copy()
    idx = np.indices((n,) * D).sum(axis=0)
    for p in range(L.P):
        d = np.zeros((n,) * D)
        ghosts, bs, rh2s = [], [], []
        for a in range(D):
            ax = _ax(L, a)
            blo, bhi = _beta_sides(L, beta, p, a)
            kap = [2.0 if isdir[p, 2 * a + k] else (0.0 if isneu[p, 2 * a + k] else 1.0) for k in (0, 1)]
            w_lo, w_hi = _face_weights(L, p, a, kap[0], kap[1])
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
        cur = U[p].copy()
        for colour in (0, 1):
            o = np.zeros((n,) * D)
            for a in range(D):
                ax = _ax(L, a)
                ext = np.concatenate([np.expand_dims(ghosts[a][0], ax), cur, np.expand_dims(ghosts[a][1], ax)], axis=ax)
                o += bs[a][0] * np.take(ext, np.arange(0, n), axis=ax) * rh2s[a]
                o += bs[a][1] * np.take(ext, np.arange(2, n + 2), axis=ax) * rh2s[a]
            new = (o - F[p]) / d
            mask = (idx & 1) == colour
            cur[mask] = new[mask]
        out[p] = cur
    return out.ravel()


def restrict_faces(F, C, beta):
    """beta of the fine level F -> beta of the coarse level C"""
    n, D = F.n, F.dim
    lo, hi = beta
    clo, chi = np.zeros((C.P, D) + (n,) * D), np.zeros((C.P, D) + (n,) * (D - 1))
    parent, orth = F.a["parent"], F.a["orth_on_parent"]
    for pc in range(C.P):
        kids = [pf for pf in range(F.P) if parent[pf] == pc]
        if len(kids) == 1 and orth[kids[0]] < 0:
            clo[pc], chi[pc] = lo[kids[0]], hi[kids[0]]
            continue
        assert len(kids) == 1 << D
        for a in range(D):
            ax = D - 1 - a
            fine = np.zeros([2 * n + 1 if i == ax else 2 * n for i in range(D)])
            for pf in sorted(kids, key=lambda q: (orth[q] >> a) & 1):  # (the mid-plane is the upper child's plane 0)
                o = orth[pf]
                sl = [None] * D
                for b in range(D):
                    ob = (o >> b) & 1
                    sl[D - 1 - b] = slice(ob * n, ob * n + n + 1) if b == a else slice(ob * n, ob * n + n)
                fine[tuple(sl)] = np.concatenate([lo[pf, a], np.expand_dims(hi[pf, a], ax)], axis=ax)
            planes = np.take(fine, np.arange(0, 2 * n + 1, 2), axis=ax)  # the fine planes 2 I
            others = [i for i in range(D) if i != ax]
            low = others[-1]  # the lower remaining axis runs fastest: the last numpy axis that is not ax
            s = np.take(planes, np.arange(0, 2 * n, 2), axis=low) + np.take(planes, np.arange(1, 2 * n, 2), axis=low)
            if D == 3:
                high = others[0]
                s = (np.take(s, np.arange(0, 2 * n, 2), axis=high) + np.take(s, np.arange(1, 2 * n, 2), axis=high)) * 0.25
            else:
                s = s * 0.5
            clo[pc, a] = np.take(s, np.arange(n), axis=ax)
            chi[pc, a] = np.take(s, n, axis=ax)
    return clo, chi


def restrict_all(levels, beta0):
    betas = [beta0]
    for l in range(len(levels) - 1):
        betas.append(restrict_faces(levels[l], levels[l + 1], betas[-1]))
    return betas


def cycle(levels, betas, f, prolong, smoother=2, pre=1, post=1, coarse=1, mid=1, cycle_type=0, omega=6.0 / 7.0):
    """prolong_util.cycle with A_b and its sweeps; the coarsest level runs `coarse` sweeps of the smoother (no exact solve).
    smoother: 1 Jacobi, 2 patch-local RB-GS -- the numbers of TE_SMOOTH_*."""
    nl = len(levels)

    def smooth(l, f, u):
        if smoother == 1:
            return jacobi(levels[l], betas[l], f, u, omega)
        return rbgs(levels[l], betas[l], f, u)

    def visit(l, f, u):
        L = levels[l]
        if l == nl - 1:
            for _ in range(coarse):
                u = smooth(l, f, u)
            return u

        def descend(u):
            r = -1 * apply(L, betas[l], u) + f
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


def bicgstab(levels, betas, b, prolong, max_it=100, tol=1e-12, **kw):
    """prolong_util.bicgstab with A_b, right-preconditioned by the composed cycle -> (x, iterations)"""
    L = levels[0]
    A = lambda v: apply(L, betas[0], v)
    M = lambda v: cycle(levels, betas, v, prolong, **kw)
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


def face_centres(t, n, dim):
    """t = Hierarchy.tables(level): the coordinates of the face centres, in beta's layout -> (lo[P, dim, coordinate, n..n], hi[...])"""
    P = len(t["id"])
    lo = np.zeros((P, dim, dim) + (n,) * dim)
    hi = np.zeros((P, dim, dim) + (n,) * (dim - 1))
    for p in range(P):
        h = t["lengths"][p] / n
        cell = [t["starts"][p][b] + (np.arange(n) + 0.5) * h[b] for b in range(dim)]
        for a in range(dim):
            ax = dim - 1 - a
            for b in range(dim):
                shape = [1] * dim
                shape[dim - 1 - b] = n
                coord = (cell[b] - 0.5 * h[b] if b == a else cell[b]).reshape(shape)  # the lower a-face: half a cell down along a
                lo[p, a, b] = np.broadcast_to(coord, (n,) * dim)
                if b == a:
                    hi[p, a, b] = t["starts"][p][a] + t["lengths"][p][a]
                else:
                    hi[p, a, b] = np.take(lo[p, a, b], 0, axis=ax)
    return lo, hi


def beta_from(t, n, dim, fn):
    """fn(x, y[, z]) evaluated at the face centres of level tables t -> (lo, hi)"""
    clo, chi = face_centres(t, n, dim)
    lo = np.stack([np.stack([fn(*[clo[p, a, b] for b in range(dim)]) for a in range(dim)]) for p in range(len(clo))])
    hi = np.stack([np.stack([fn(*[chi[p, a, b] for b in range(dim)]) for a in range(dim)]) for p in range(len(chi))])
    return lo + 0.0, hi + 0.0


def cell_centres(t, n, dim):
    """[P, coordinate, n..n]"""
    P = len(t["id"])
    out = np.zeros((P, dim) + (n,) * dim)
    for p in range(P):
        h = t["lengths"][p] / n
        for b in range(dim):
            shape = [1] * dim
            shape[dim - 1 - b] = n
            out[p, b] = np.broadcast_to((t["starts"][p][b] + (np.arange(n) + 0.5) * h[b]).reshape(shape), (n,) * dim)
    return out


def boundary_centres(L, t):
    """the centres of the physical faces in boundary-vector order -> [num_bfaces * nf, dim]"""
    n, D = L.n, L.dim
    clo, chi = face_centres(t, n, D)
    out = []
    for p in range(L.P):
        for s in range(2 * D):
            if L.a["nbr_kind"][p, s] != 0:
                continue
            a = s >> 1
            pts = [chi[p, a, b] if s & 1 else np.take(clo[p, a, b], 0, axis=D - 1 - a) for b in range(D)]
            out.append(np.stack([q.ravel() for q in pts], axis=1))
    return np.concatenate(out) if out else np.zeros((0, D))


def boundary_rhs(L, beta, bd):
    """the right-hand-side terms of inhomogeneous boundary data under A_b: -div(beta (.) grad(0, bdata))"""
    lo, hi = pu.level_grad(L, np.zeros(L.size), bd)
    return -pu.level_div(L, lo * beta[0], hi * beta[1])


# ---- the problems of the tests
def manufactured2d():
    """beta = exp(x + y), u = sin(2x + 0.3) sin(3y + 0.1), F = div(beta grad u)"""
    beta = lambda x, y: np.exp(x + y)
    u = lambda x, y: np.sin(2 * x + 0.3) * np.sin(3 * y + 0.1)
    F = lambda x, y: np.exp(x + y) * (-13.0 * u(x, y) + 2 * np.cos(2 * x + 0.3) * np.sin(3 * y + 0.1) + 3 * np.sin(2 * x + 0.3) * np.cos(3 * y + 0.1))
    return beta, u, F


def manufactured_problem(H, levels, n, dim, beta_fn, u_fn, F_fn):
    """-> (betas per level, right-hand side with the boundary terms of the b_beta recipe, exact solution at the cell centres)"""
    L, t = levels[0], H.tables(0)
    betas = restrict_all(levels, beta_from(t, n, dim, beta_fn))
    cc = cell_centres(t, n, dim)
    exact = np.concatenate([u_fn(*[cc[p, b] for b in range(dim)]).ravel() for p in range(L.P)])
    F = np.concatenate([F_fn(*[cc[p, b] for b in range(dim)]).ravel() for p in range(L.P)])
    bc = boundary_centres(L, t)
    bd = u_fn(*[bc[:, b] for b in range(dim)])
    return betas, F + boundary_rhs(L, betas[0], bd), exact


def smooth_beta(*x):
    out = 1.0
    for i, xi in enumerate(x):
        out = out * np.sin(2 * np.pi * (xi + 0.1 * i))
    return 1.0 + 0.5 * out


def jump_beta(*x):
    r2 = sum((xi - 0.5) ** 2 for xi in x)
    return np.where(r2 < 0.3 ** 2, 100.0, 1.0)
