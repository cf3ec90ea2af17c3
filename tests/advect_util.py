"""The numpy statement of te_advect_flux, te_advect, te_faces_match and te_faces_max_rate (include/te_hip.h) on
an oracle level: the specification the device kernels are held to, written from the rules, not from the kernels. Layouts are
projection_util's: a face vector is a pair (lo[P, dim, n..n], hi[P, dim, n..n (dim-1 axes)]), a boundary vector one block of
n^(dim-1) values per physical face in (patch, side) order, laid out like hi[p, a].

    flux of a face     lo, hi = the operands on the lower- and the upper-coordinate side, U = the patch's stored entry:
                       s = lo where U >= 0.0 else hi, F = U * s
    same level         the neighbour's facing cell
    physical face      outside: the boundary vector's entry, or the cell just inside; inside: that cell
    neighbour coarser (kind 2)   the other operand is the coarse cell of its facing layer that covers the face
    neighbours finer (kind 3)    ((F00 + F10) + (F01 + F11)) * 0.25 of the fine-side fluxes of the covering fine faces, each from the
                                 fine patch's copy of U, its facing-layer cell and this coarse cell; first index along the face's
                                 lower remaining axis; 2D (F0 + F1) * 0.5. The coarse copy of U is not read.
    faces_match        the kind 3 entries <- the same mean of the fine copies, everything else unchanged
    advect             c - div(alpha, F) with projection_util's divergence (the device's roundings are te_divergence's)
    max_rate           max |U_a| / h_a over all stored entries"""
import numpy as np

from tests import density_util as du, projection_util as pu


def flux(U, lo, hi):
    return U * np.where(U >= 0.0, lo, hi)


def mean_of_fine(Ff, dim):
    """a fine face block -> the means over the 2^(dim-1) fine faces of each coarse face (half the size per axis)"""
    if dim == 2:
        return (Ff[0::2] + Ff[1::2]) * 0.5
    return ((Ff[0::2, 0::2] + Ff[0::2, 1::2]) + (Ff[1::2, 0::2] + Ff[1::2, 1::2])) * 0.25


def quadrant(n, dim, qd):
    h = n // 2
    qa, qb = qd & 1, qd >> 1
    return (slice(qa * h, (qa + 1) * h),) if dim == 2 else (slice(qb * h, (qb + 1) * h), slice(qa * h, (qa + 1) * h))


def advect_flux(L, U, c, cb=None, match=True):
    """U = (lo, hi) -> F = (lo, hi). match=False is the negative control: the coarse side of a coarse/fine face forms a flux of its
    own, from its own copy of U and te_faces_from_cells' four-cell average."""
    n, dim = L.n, L.dim
    C = np.asarray(c, np.float64).reshape((L.P,) + (n,) * dim)
    Ulo, Uhi = U
    fshape = (n,) * (dim - 1)
    nf = n ** (dim - 1)
    kind, nbr = L.a["nbr_kind"], L.a["nbr"]
    bidx = pu.bface_index(kind)
    lo = np.zeros((L.P, dim) + (n,) * dim)
    hi = np.zeros((L.P, dim) + fshape)
    for p in range(L.P):
        for a in range(dim):
            ax = dim - 1 - a
            sl = [slice(None)] * dim
            sl[ax] = slice(1, None)
            lo[p, a][tuple(sl)] = flux(Ulo[p, a][tuple(sl)], np.take(C[p], np.arange(0, n - 1), axis=ax), np.take(C[p], np.arange(1, n), axis=ax))
            for upper in (0, 1):
                s = 2 * a + upper
                m = du.layer(C, L, p, s)
                Uf = du.side_face(Ulo, Uhi, p, s, dim)
                k = kind[p, s]
                if k == 3 and match:
                    val = np.zeros(fshape)
                    for qd in range(1 << (dim - 1)):
                        f = int(nbr[p, s, qd])
                        Q = quadrant(n, dim, qd)
                        mq = m[Q]
                        for d in range(dim - 1):
                            mq = np.repeat(mq, 2, axis=d)  # the coarse cell behind each fine face
                        fc, Ufine = du.layer(C, L, f, s ^ 1), du.side_face(Ulo, Uhi, f, s ^ 1, dim)
                        val[Q] = mean_of_fine(flux(Ufine, mq, fc) if upper else flux(Ufine, fc, mq), dim)
                else:
                    if k == 0:
                        o = m if cb is None else np.asarray(cb)[bidx[p, s] * nf:(bidx[p, s] + 1) * nf].reshape(fshape)
                    else:
                        o = du.other_operand(L, C, p, s)
                    val = flux(Uf, m, o) if upper else flux(Uf, o, m)
                if upper:
                    hi[p, a] = val
                else:
                    sl = [slice(None)] * dim
                    sl[ax] = 0
                    lo[p, a][tuple(sl)] = val
    return lo, hi


def faces_match(L, F):
    """(lo, hi) -> (lo, hi), copies: the coarse side of every coarse/fine face <- the mean of the covering fine copies"""
    n, dim = L.n, L.dim
    lo, hi = F[0].copy(), F[1].copy()
    kind, nbr = L.a["nbr_kind"], L.a["nbr"]
    for p in range(L.P):
        for s in range(2 * dim):
            if kind[p, s] != 3:
                continue
            a = s >> 1
            val = np.zeros((n,) * (dim - 1))
            for qd in range(1 << (dim - 1)):
                val[quadrant(n, dim, qd)] = mean_of_fine(du.side_face(F[0], F[1], int(nbr[p, s, qd]), s ^ 1, dim), dim)
            if s & 1:
                hi[p, a] = val
            else:
                sl = [slice(None)] * dim
                sl[dim - 1 - a] = 0
                lo[p, a][tuple(sl)] = val
    return lo, hi


def advect(L, U, c, alpha, cb=None, match=True):
    """c - alpha div(U c_upwind) -> (the result, the flux it used)"""
    F = advect_flux(L, U, c, cb, match)
    return np.asarray(c, np.float64) - pu.level_div(L, F[0], F[1], alpha), F


def max_rate(L, U):
    h = L.a["h"]
    r = 0.0
    for p in range(L.P):
        for a in range(L.dim):
            r = max(r, np.abs(U[0][p, a]).max() / h[p, a], np.abs(U[1][p, a]).max() / h[p, a])
    return float(r)


# ---- what the conservation statement needs
def cell_volumes(L):
    """one volume per cell, in the order of a domain vector"""
    return np.repeat(np.prod(L.a["h"][:, :L.dim], axis=1), L.n ** L.dim)


def flux_area_sum(L, F):
    """sum over all stored entries of |F| * (area of the face)"""
    h = L.a["h"]
    t = 0.0
    for p in range(L.P):
        vol = float(np.prod(h[p, :L.dim]))
        for a in range(L.dim):
            t += (np.abs(F[0][p, a]).sum() + np.abs(F[1][p, a]).sum()) * (vol / h[p, a])
    return t


def one_way(U):
    """|U| with one sign per axis (+x, -y, +z): both signs occur, and no cell has outflow through both of its faces along an axis --
    the class of fields (it contains every discretely divergence-free one in the sense that matters: a cell's outflow rates sum to at
    most dim * rate) for which alpha * dim * rate <= 1 keeps the update non-negative"""
    lo, hi = np.abs(U[0]), np.abs(U[1])
    for a in range(lo.shape[1]):
        if a == 1:
            lo[:, a] *= -1.0
            hi[:, a] *= -1.0
    return lo, hi


def single_valued(L, U, zero_physical=False):
    """a copy of U = (lo, hi) whose two copies of every same-level face agree (the upper patch takes the lower patch's HI entry);
    zero_physical: and with U = 0 on the physical faces"""
    n, dim = L.n, L.dim
    lo, hi = U[0].copy(), U[1].copy()
    for p, a, q in du.same_level_pairs(L):
        sl = [slice(None)] * dim
        sl[dim - 1 - a] = 0
        lo[q, a][tuple(sl)] = hi[p, a]
    if zero_physical:
        kind = L.a["nbr_kind"]
        for p in range(L.P):
            for s in range(2 * dim):
                if kind[p, s] == 0:
                    if s & 1:
                        hi[p, s >> 1] = 0.0
                    else:
                        sl = [slice(None)] * dim
                        sl[dim - 1 - (s >> 1)] = 0
                        lo[p, s >> 1][tuple(sl)] = 0.0
    return lo, hi
