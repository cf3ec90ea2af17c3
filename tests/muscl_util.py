"""The numpy statement of te_cell_slopes, te_advect_flux_muscl and te_advect_muscl (include/te_hip.h) on an
oracle level: the specification the device kernels are held to, written from the rules, not from the kernels. Layouts and helpers
are advect_util's, density_util's and projection_util's; a slope vector is a cell vector.

    slope of a cell along axis a    dm = c - m, dp = p - c, with m and p the operands beyond the cell's lower and upper a-face: the
                                    same-level neighbour's facing cell; on a physical face the boundary vector's entry, or without
                                    cb the cell itself; the covering coarse cell, raw, where the neighbour is coarser;
                                    density_util.other_operand's average of the covering fine cells where the neighbours are finer
      ZERO (0)      S = 0.0
      MINMOD (1)    S = (dm*dp > 0.0) ? (fabs(dm) < fabs(dp) ? dm : dp) : 0.0
      MC (2)        t = 0.5*(dm + dp), w = fmin(fmin(2.0*fabs(dm), 2.0*fabs(dp)), fabs(t)), S = (dm*dp > 0.0) ? copysign(w, dm) : 0.0
      CENTRAL (3)   S = 0.5*(dm + dp)
    flux of a face                  advect_util.flux (s = lo where U >= 0.0 else hi, F = U * s) with the cell operands replaced by
                                    edge states: a cell on the lower side of the face contributes lo = c + 0.5*S_a, a cell on the
                                    upper side hi = c - 0.5*S_a; an operand that is not a cell of this level (the boundary datum, the
                                    own cell standing in for it, the raw coarse cell, the coarse cell on the coarse side) enters as
                                    it is
    neighbour coarser (kind 2)      flux(U_f, C, m - 0.5*S) on a lower face, flux(U_f, m + 0.5*S, C) on an upper one
    neighbours finer (kind 3)       advect_util.mean_of_fine of those fine-side values, formed from the fine patch's own U, m, S and
                                    this coarse cell; the coarse copy of U is not read
    advect                          c - div(alpha, F) with projection_util's divergence

Every operation is rounded on its own; numpy evaluates the expressions above as they are written."""
import numpy as np

from tests import advect_util as au, density_util as du, projection_util as pu

ZERO, MINMOD, MC, CENTRAL = 0, 1, 2, 3
KINDS = (ZERO, MINMOD, MC, CENTRAL)
LIMITED = (ZERO, MINMOD, MC)  # the kinds with the positivity guarantee


def slope(kind, dm, dp):
    if kind == ZERO:
        return np.zeros_like(dm)
    if kind == CENTRAL:
        return 0.5 * (dm + dp)
    same = dm * dp > 0.0
    if kind == MINMOD:
        return np.where(same, np.where(np.abs(dm) < np.abs(dp), dm, dp), 0.0)
    assert kind == MC
    t = 0.5 * (dm + dp)
    w = np.minimum(np.minimum(2.0 * np.abs(dm), 2.0 * np.abs(dp)), np.abs(t))
    return np.where(same, np.copysign(w, dm), 0.0)


def outside_operand(L, C, p, s, cb, bidx):
    """what stands beyond side s of patch p: te_faces_from_cells' and te_advect_flux's operand, as a face block"""
    n, dim = L.n, L.dim
    if L.a["nbr_kind"][p, s] == 0:
        nf = n ** (dim - 1)
        return du.layer(C, L, p, s) if cb is None else np.asarray(cb)[bidx[p, s] * nf:(bidx[p, s] + 1) * nf].reshape((n,) * (dim - 1))
    return du.other_operand(L, C, p, s)


def cell_slopes(L, c, kind, cb=None):
    """-> S[dim][P, n..n]: S[a] is the slope along axis a (a = 0 is x, the fastest index)"""
    n, dim = L.n, L.dim
    C = np.asarray(c, np.float64).reshape((L.P,) + (n,) * dim)
    bidx = pu.bface_index(L.a["nbr_kind"])
    S = np.zeros((dim,) + C.shape)
    for p in range(L.P):
        for a in range(dim):
            ax = dim - 1 - a
            below = np.expand_dims(outside_operand(L, C, p, 2 * a, cb, bidx), ax)
            above = np.expand_dims(outside_operand(L, C, p, 2 * a + 1, cb, bidx), ax)
            ext = np.concatenate([below, C[p], above], axis=ax)
            mid, lo, hi = (np.take(ext, np.arange(k, k + n), axis=ax) for k in (1, 0, 2))
            S[a, p] = slope(kind, mid - lo, hi - mid)
    return S


def advect_flux(L, U, c, kind, cb=None, match=True):
    """U = (lo, hi) -> F = (lo, hi). match=False is the negative control: the coarse side of a coarse/fine face forms a flux of its
    own, from its own copy of U, its own edge state and te_faces_from_cells' four-cell average."""
    n, dim = L.n, L.dim
    C = np.asarray(c, np.float64).reshape((L.P,) + (n,) * dim)
    S = cell_slopes(L, c, kind, cb)
    Ulo, Uhi = U
    fshape = (n,) * (dim - 1)
    kinds, nbr = L.a["nbr_kind"], L.a["nbr"]
    bidx = pu.bface_index(kinds)
    lo = np.zeros((L.P, dim) + (n,) * dim)
    hi = np.zeros((L.P, dim) + fshape)
    for a in range(dim):
        ax = dim - 1 - a
        up_edge, low_edge = C + 0.5 * S[a], C - 0.5 * S[a]  # what a cell contributes to its upper and to its lower a-face
        for p in range(L.P):
            sl = [slice(None)] * dim
            sl[ax] = slice(1, None)
            lo[p, a][tuple(sl)] = au.flux(Ulo[p, a][tuple(sl)], np.take(up_edge[p], np.arange(0, n - 1), axis=ax),
                                          np.take(low_edge[p], np.arange(1, n), axis=ax))
            for upper in (0, 1):
                s = 2 * a + upper
                me = du.layer(up_edge if upper else low_edge, L, p, s)  # the facing cells' edge states on this face
                Uf = du.side_face(Ulo, Uhi, p, s, dim)
                k = kinds[p, s]
                if k == 3 and match:
                    m = du.layer(C, L, p, s)
                    val = np.zeros(fshape)
                    for qd in range(1 << (dim - 1)):
                        f = int(nbr[p, s, qd])
                        Q = au.quadrant(n, dim, qd)
                        mq = m[Q]
                        for d in range(dim - 1):
                            mq = np.repeat(mq, 2, axis=d)  # the coarse cell behind each fine face, raw
                        fe = du.layer(low_edge if upper else up_edge, L, f, s ^ 1)  # the fine cells' edge states on the face
                        Ufine = du.side_face(Ulo, Uhi, f, s ^ 1, dim)
                        val[Q] = au.mean_of_fine(au.flux(Ufine, mq, fe) if upper else au.flux(Ufine, fe, mq), dim)
                else:
                    if k == 1:  # the neighbour's facing cells are cells of this level: their edge states
                        o = du.layer(low_edge if upper else up_edge, L, int(nbr[p, s, 0]), s ^ 1)
                    else:
                        o = outside_operand(L, C, p, s, cb, bidx)
                    val = au.flux(Uf, me, o) if upper else au.flux(Uf, o, me)
                if upper:
                    hi[p, a] = val
                else:
                    sl = [slice(None)] * dim
                    sl[ax] = 0
                    lo[p, a][tuple(sl)] = val
    return lo, hi


def advect(L, U, c, alpha, kind, cb=None, match=True):
    """c - alpha div(F) -> (the result, the flux it used)"""
    F = advect_flux(L, U, c, kind, cb, match)
    return np.asarray(c, np.float64) - pu.level_div(L, F[0], F[1], alpha), F


def positivity_factor(L):
    """K in the positivity bound alpha * K * dim * rate <= 1: 2 on a level without coarse/fine faces, 2.5 on one
    with them -- a coarse cell loses its RAW value through a coarse/fine face (at half the rate) beside up to 2c through the
    opposite face, whose edge state is formed from the fine cells' average beyond the coarse/fine face"""
    return 2.5 if (L.a["nbr_kind"] == 3).any() else 2.0
