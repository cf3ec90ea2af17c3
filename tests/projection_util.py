"""The numpy statement of the MAC gradient and divergence (include/te_hip.h te_gradient / te_divergence) that the projection
tests compare against, and the face-vector layout helpers that go with it.

    interior face              G = (u[c] - u[c - e_a]) / h_a
    patch face, neighbour      2 (m - gamma) / h_a below, 2 (gamma - m) / h_a above, gamma = the interface value of
                               SchurHelper::interpolateToInterface (the oracle's orc.interp, or the reference's golden gamma)
    physical Dirichlet face    ghost 2 g - m: 2 (m - g) / h_a below, 2 (g - m) / h_a above
    physical Neumann face      G = g_n
    divergence                 out[c] = alpha * sum_a (U_a(upper face of c) - U_a(lower face of c)) / h_a

lo[p, a] has the shape of a patch (numpy index order z, y, x): the component on the lower a-face of each cell; hi[p, a] has the
shape of a face (the remaining axes, slowest first): the component on the patch's upper a-face. Boundary data: one block of
n^(dim-1) values per physical face in (patch, side) order, laid out like hi[p, a]."""
import numpy as np

from oracle import oracle as orc

EPS = np.finfo(np.float64).eps


def bface_index(nbr_kind):
    """[P][2 dim] number of the physical face in (patch, side) order, -1 on a face with a neighbour"""
    phys = np.asarray(nbr_kind) == 0
    out = np.full(phys.shape, -1, np.int64)
    out[phys] = np.arange(int(phys.sum()))
    return out


def grad(u, h, n, dim, kind, neu, gamma, iidx, bd=None):
    P = len(kind)
    U = np.asarray(u).reshape((P,) + (n,) * dim)
    nf = n ** (dim - 1)
    fshape = (n,) * (dim - 1)
    bidx = bface_index(kind)
    lo = np.zeros((P, dim) + (n,) * dim)
    hi = np.zeros((P, dim) + fshape)
    for p in range(P):
        for a in range(dim):
            ax = dim - 1 - a  # numpy axis of coordinate a inside a patch
            up = U[p]
            sl = [slice(None)] * dim
            sl[ax] = slice(1, None)
            lo[p, a][tuple(sl)] = np.diff(up, axis=ax) / h[p, a]
            for upper in (0, 1):
                s = 2 * a + upper
                m = np.take(up, n - 1 if upper else 0, axis=ax)
                if kind[p, s] != 0:
                    g = gamma[iidx[p, s] * nf:(iidx[p, s] + 1) * nf].reshape(fshape)
                    val = 2 * (g - m) / h[p, a] if upper else 2 * (m - g) / h[p, a]
                else:
                    g = np.zeros(fshape) if bd is None else bd[bidx[p, s] * nf:(bidx[p, s] + 1) * nf].reshape(fshape)
                    if (neu[p] >> s) & 1:
                        val = g.copy()
                    else:
                        val = 2 * (g - m) / h[p, a] if upper else 2 * (m - g) / h[p, a]
                if upper:
                    hi[p, a] = val
                else:
                    sl = [slice(None)] * dim
                    sl[ax] = 0
                    lo[p, a][tuple(sl)] = val
    return lo, hi


def div(lo, hi, h, n, dim, alpha=1.0):
    P = len(lo)
    out = np.zeros((P,) + (n,) * dim)
    for p in range(P):
        for a in range(dim):
            ax = dim - 1 - a
            full = np.concatenate([lo[p, a], np.expand_dims(hi[p, a], ax)], axis=ax)
            out[p] += np.diff(full, axis=ax) / h[p, a]
    return alpha * out.ravel()


def boundary_rhs(h, n, dim, kind, neu, bd):
    """what te_add_boundary_rhs(bd, .) adds to a zero vector: -2 g / h^2 on Dirichlet faces, +g_n / h below and -g_n / h above on
    Neumann faces"""
    P = len(kind)
    nf = n ** (dim - 1)
    bidx = bface_index(kind)
    out = np.zeros((P,) + (n,) * dim)
    for p in range(P):
        for s in range(2 * dim):
            if kind[p, s] != 0:
                continue
            a, upper = s >> 1, s & 1
            g = bd[bidx[p, s] * nf:(bidx[p, s] + 1) * nf].reshape((n,) * (dim - 1))
            sl = [slice(None)] * dim
            sl[dim - 1 - a] = n - 1 if upper else 0
            if (neu[p] >> s) & 1:
                out[p][tuple(sl)] += (-g if upper else g) / h[p, a]
            else:
                out[p][tuple(sl)] += -2 * g / h[p, a] ** 2
    return out.ravel()


def level_grad(L, u, bd=None):
    """the statement on an oracle level, gamma from the oracle's interpolation"""
    a = L.a
    return grad(u, a["h"], L.n, L.dim, a["nbr_kind"], a["neumann"], orc.interp(L, u), L.iface_index(), bd)


def level_div(L, lo, hi, alpha=1.0):
    return div(lo, hi, L.a["h"], L.n, L.dim, alpha)


def level_boundary_rhs(L, bd):
    a = L.a
    return boundary_rhs(a["h"], L.n, L.dim, a["nbr_kind"], a["neumann"], bd)


def num_bfaces(L):
    return int((L.a["nbr_kind"] == 0).sum())


def face_size(n, dim):
    return dim * n ** dim + dim * n ** (dim - 1)


def pack(lo, hi):
    """(lo, hi) -> the flat host array of a face vector"""
    P = len(lo)
    return np.concatenate([lo.reshape(P, -1), hi.reshape(P, -1)], axis=1).ravel()


def unpack(a, n, dim):
    """the flat host array of a face vector -> (lo[P, dim, n..n], hi[P, dim, n..n (dim-1 axes)]) (copies)"""
    per = np.asarray(a).reshape(-1, face_size(n, dim))
    nlo = dim * n ** dim
    return per[:, :nlo].reshape((-1, dim) + (n,) * dim).copy(), per[:, nlo:].reshape((-1, dim) + (n,) * (dim - 1)).copy()


def grad_tol(L, u, bd=None):
    """a few ulps of sum |coef| |u|: 5 / h is the largest coefficient sum, on the fine side of a coarse/fine face
    (2 / h (1 + 14 / 12 + 4 / 12))"""
    big = max(np.abs(u).max(), np.abs(bd).max() if bd is not None and bd.size else 0.0, 1e-300)
    return 32 * EPS * 5 / L.a["h"].min() * big


def div_tol(L, U):
    return 32 * EPS * 2 * L.dim / L.a["h"].min() * max(np.abs(U).max(), 1e-300)
