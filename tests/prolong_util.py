"""Test infrastructure of the linear interpolator (TE_INTERP_LINEAR): the numpy statement of its semantics -- the specification
the device kernels are held to -- and a cycle / BiCGStab composed in Python (tests/cycle_util.py's driver) from the oracle's pieces,
so that the prolongation can be swapped. With orc.prolong_add the composition IS orc.cycle (tests/test_prolong_host.py asserts
equality to 0.0)."""
import numpy as np

from oracle import oracle as orc
from tests import cycle_util


def extended(C, e):
    """C: orc.Level (coarse), e: flat vector -> [P, n+2, ..] (numpy axis of coordinate a = D-1-a): the patches' values extended to
    indices -1 .. n per axis. One axis out of range: the ghost the operator's stencil reads there for homogeneous data (2 gamma - m
    on a face with a neighbour, -m Dirichlet, +m Neumann); k >= 2 axes out: the sum of the face ghosts of the clamped cell m through
    the out-of-range axes, in ascending order, minus (k - 1) m."""
    D, n = C.dim, C.n
    ev = e.reshape((C.P,) + (n,) * D)
    E = np.zeros((C.P,) + (n + 2,) * D)
    gam, ii, kind, neu = orc.interp(C, e), C.iface_index(), C.a["nbr_kind"], C.a["neumann"]
    cl = np.clip(np.arange(-1, n + 1), 0, n - 1)
    for p in range(C.P):
        tot = -(D - 1) * ev[p][np.ix_(*([cl] * D))]
        for a in range(D):
            ax = D - 1 - a
            Pa = np.zeros([n + 2 if i == ax else n for i in range(D)])
            sl = [slice(None)] * D
            sl[ax] = slice(1, -1)
            Pa[tuple(sl)] = ev[p]
            for up in (0, 1):
                s = 2 * a + up
                m = np.take(ev[p], n - 1 if up else 0, axis=ax)
                if kind[p, s] != 0:
                    g = 2 * gam[ii[p, s] * C.nf:(ii[p, s] + 1) * C.nf].reshape((n,) * (D - 1)) - m
                else:
                    g = m if (neu[p] >> s) & 1 else -m
                sl = [slice(None)] * D
                sl[ax] = -1 if up else 0
                Pa[tuple(sl)] = g
            tot = tot + Pa[np.ix_(*[np.arange(n + 2) if i == ax else cl for i in range(D)])]
        E[p] = tot
    return E


def prolong_linear_add(F, C, e, u):
    """F: fine orc.Level, C: coarse; returns u + P_linear e (a patch that copies through receives u + e)"""
    D, n = F.dim, F.n
    E = extended(C, e)
    out = u.reshape((F.P,) + (n,) * D).copy()
    i = np.arange(n)
    for pf in range(F.P):
        pc, o = F.a["parent"][pf], F.a["orth_on_parent"][pf]
        if o < 0:
            out[pf] += e.reshape((C.P,) + (n,) * D)[pc]
            continue
        blk = E[pc]
        for a in range(D):
            c = (i + ((o >> a) & 1) * n) // 2
            nb = c + np.where(i % 2 == 0, -1, 1)
            blk = 0.75 * np.take(blk, c + 1, axis=D - 1 - a) + 0.25 * np.take(blk, nb + 1, axis=D - 1 - a)
        out[pf] += blk
    return out.ravel()


def direct(F, C, e, u):
    return orc.prolong_add(F, C, e, u)


def cycle(levels, f, prolong, smoother=2, omega=6.0 / 7.0, exact_coarse=1, **kw):
    """oracle/te_oracle.cpp visit() statement by statement (cycle_util.visit with the oracle's operator and sweeps), the prolongation
    a parameter. smoother: 0 block Jacobi (exact patch solves), 1 Jacobi, 2 patch-local RB-GS -- the numbers of TE_SMOOTH_*.
    kw: pre, post, coarse, mid, cycle_type."""
    nl = len(levels)

    def smooth(l, f, u):
        L = levels[l]
        if smoother == 0 or (l == nl - 1 and exact_coarse and L.P == 1):
            return orc.smooth(L, f, u)
        if smoother == 1:
            return orc.jacobi(L, f, u, omega)
        return orc.patch_rbgs(L, f, u)

    return cycle_util.cycle(levels, f, lambda l, u: orc.apply(levels[l], u), smooth, prolong, **kw)


def reductions(levels, f, prolong, cycles=8, **kw):
    """residual reduction |r_k| / |r_k-1| of the stationary iteration u += M (f - A u), k = 1 .. cycles"""
    L = levels[0]
    u = np.zeros(L.size)
    r = np.array(f, dtype=np.float64)
    out = []
    for _ in range(cycles):
        u = u + cycle(levels, r, prolong, **kw)
        rn = f - orc.apply(L, u)
        out.append(np.linalg.norm(rn) / np.linalg.norm(r))
        r = rn
    return out


def bicgstab(levels, b, prolong, max_it=100, tol=1e-12, **kw):
    """oracle/te_oracle.cpp orc_bicgstab (BiCGStab.h:45-106), right-preconditioned by the composed cycle -> (x, iterations)"""
    return cycle_util.bicgstab(lambda v: orc.apply(levels[0], v), lambda v: cycle(levels, v, prolong, **kw), b, max_it, tol)
