"""The numpy statement of te_faces_from_cells, te_project_weighted and te_add_boundary_rhs_weighted (include/te_hip.h, DESIGN.md
section 21) on an oracle level: the specification the device kernels are held to. Layouts are projection_util's: a face vector is a
pair (lo[P, dim, n..n], hi[P, dim, n..n (dim-1 axes)]), a boundary vector one block of n^(dim-1) values per physical face in
(patch, side) order, laid out like hi[p, a].

    face value      lo, hi = the operands on the lower- and the upper-coordinate side of the face
                    MEAN (lo + hi) * 0.5, HARMONIC (2.0 * (lo * hi)) / (lo + hi), RECIP_MEAN 2.0 / (lo + hi)
    physical face   v = the boundary vector's entry, or the cell just inside: v (MEAN, HARMONIC), 1.0 / v (RECIP_MEAN)
    same level      the neighbour's facing cell
    neighbour coarser (kind 2)   the coarse cell of its facing layer at ((a + (q & 1 ? n : 0)) / 2, (b + (q & 2 ? n : 0)) / 2)
    neighbours finer (kind 3)    ((f00 + f10) + (f01 + f11)) * 0.25 of the facing layer's four cells that cover the coarse cell,
                                 first index along the face's lower remaining axis; 2D (f0 + f1) * 0.5
    project_weighted             U - alpha * (w * G), G = projection_util.level_grad
    boundary_rhs_weighted        b = w_face * b, then Dirichlet f -= 2 b / (h h), Neumann f += b / h below, f -= b / h above, the terms
                                 of a cell applied in side order"""
import numpy as np

from tests import projection_util as pu

MEAN, HARMONIC, RECIP_MEAN = 0, 1, 2
MODES = (MEAN, HARMONIC, RECIP_MEAN)


def face_value(mode, lo, hi):
    s = lo + hi
    if mode == MEAN:
        return s * 0.5
    if mode == HARMONIC:
        return (2.0 * (lo * hi)) / s
    return 2.0 / s


def phys_value(mode, v):
    return 1.0 / v if mode == RECIP_MEAN else v + 0.0


def layer(C, L, p, s):
    """the cells of patch p along side s, in the layout of a face block (the remaining axes, slowest first)"""
    return np.take(C[p], L.n - 1 if s & 1 else 0, axis=L.dim - 1 - (s >> 1))


def other_operand(L, C, p, s):
    """what stands on the far side of side s of patch p (a side with a neighbour)"""
    n, dim = L.n, L.dim
    kind, nbr, q = L.a["nbr_kind"][p, s], L.a["nbr"][p, s], int(L.a["nbr_orth"][p, s])
    if kind == 1:
        return layer(C, L, int(nbr[0]), s ^ 1)
    h = n // 2
    if kind == 2:  # the neighbour is coarser: its cell that covers the face
        CL = layer(C, L, int(nbr[0]), s ^ 1)
        ia = (np.arange(n) + (n if q & 1 else 0)) // 2
        if dim == 2:
            return CL[ia]
        ib = (np.arange(n) + (n if q & 2 else 0)) // 2
        return CL[np.ix_(ib, ia)]
    assert kind == 3
    out = np.zeros((n,) * (dim - 1))
    for qd in range(1 << (dim - 1)):
        FL = layer(C, L, int(nbr[qd]), s ^ 1)
        qa, qb = qd & 1, qd >> 1
        if dim == 2:
            out[qa * h:(qa + 1) * h] = (FL[0::2] + FL[1::2]) * 0.5
        else:
            avg = ((FL[0::2, 0::2] + FL[0::2, 1::2]) + (FL[1::2, 0::2] + FL[1::2, 1::2])) * 0.25
            out[qb * h:(qb + 1) * h, qa * h:(qa + 1) * h] = avg
    return out


def faces_from_cells(L, c, mode, cb=None):
    n, dim = L.n, L.dim
    C = np.asarray(c, np.float64).reshape((L.P,) + (n,) * dim)
    fshape = (n,) * (dim - 1)
    nf = n ** (dim - 1)
    kind = L.a["nbr_kind"]
    bidx = pu.bface_index(kind)
    lo = np.zeros((L.P, dim) + (n,) * dim)
    hi = np.zeros((L.P, dim) + fshape)
    for p in range(L.P):
        for a in range(dim):
            ax = dim - 1 - a
            low = np.take(C[p], np.arange(0, n - 1), axis=ax)
            up = np.take(C[p], np.arange(1, n), axis=ax)
            sl = [slice(None)] * dim
            sl[ax] = slice(1, None)
            lo[p, a][tuple(sl)] = face_value(mode, low, up)
            for upper in (0, 1):
                s = 2 * a + upper
                m = layer(C, L, p, s)
                if kind[p, s] == 0:
                    v = m if cb is None else np.asarray(cb)[bidx[p, s] * nf:(bidx[p, s] + 1) * nf].reshape(fshape)
                    val = phys_value(mode, v)
                else:
                    o = other_operand(L, C, p, s)
                    val = face_value(mode, m, o) if upper else face_value(mode, o, m)
                if upper:
                    hi[p, a] = val
                else:
                    sl = [slice(None)] * dim
                    sl[ax] = 0
                    lo[p, a][tuple(sl)] = val
    return lo, hi


def project_weighted(L, U, p, w, alpha=1.0, bd=None):
    """U, w = (lo, hi) -> (lo, hi), and the gradient it used"""
    G = pu.level_grad(L, p, bd)
    return (U[0] - alpha * (w[0] * G[0]), U[1] - alpha * (w[1] * G[1])), G


def boundary_rhs_weighted(L, w, bd, f=None):
    """f (zero if None) with the weighted boundary terms folded in -> (the result, per cell |f_c| + the sum of the |terms|)"""
    n, dim = L.n, L.dim
    kind, neu, h = L.a["nbr_kind"], L.a["neumann"], L.a["h"]
    nf = n ** (dim - 1)
    bidx = pu.bface_index(kind)
    out = np.zeros((L.P,) + (n,) * dim) if f is None else np.array(f, np.float64).reshape((L.P,) + (n,) * dim)
    mag = np.abs(out)
    for p in range(L.P):
        for s in range(2 * dim):
            if kind[p, s] != 0:
                continue
            a, upper = s >> 1, s & 1
            sl = [slice(None)] * dim
            sl[dim - 1 - a] = n - 1 if upper else 0
            wf = w[1][p, a] if upper else w[0][p, a][tuple(sl)]
            b = wf * np.asarray(bd)[bidx[p, s] * nf:(bidx[p, s] + 1) * nf].reshape((n,) * (dim - 1))
            if (neu[p] >> s) & 1:
                g = b / h[p, a]
                out[p][tuple(sl)] = out[p][tuple(sl)] - g if upper else out[p][tuple(sl)] + g
                mag[p][tuple(sl)] += np.abs(g)
            else:
                t = 2 * b / (h[p, a] * h[p, a])
                out[p][tuple(sl)] = out[p][tuple(sl)] - t
                mag[p][tuple(sl)] += np.abs(t)
    return out.ravel(), mag.ravel()


def same_level_pairs(L):
    """(p, a, q): patch q is the same-level neighbour above side 2 a + 1 of patch p"""
    kind, nbr = L.a["nbr_kind"], L.a["nbr"]
    return [(p, a, int(nbr[p, 2 * a + 1, 0])) for p in range(L.P) for a in range(L.dim) if kind[p, 2 * a + 1] == 1]


def lower_face(lo, q, a, dim):
    return np.take(lo[q, a], 0, axis=dim - 1 - a)


def side_face(lo, hi, p, s, dim):
    a = s >> 1
    return hi[p, a] if s & 1 else lower_face(lo, p, a, dim)
