"""The numpy statement of the sub-patch coarse solve of the variable-coefficient path (include/te_hip.h te_gmg_set_coef_coarse,
DESIGN.md section 20), composed from tests/varcoef_util.py and tests/reaction_util.py by import.

A coarsest level of ONE patch of n^D cells is the same grid as a uniform tree of (n / s)^D patches of s^D cells. With the sub-cycle
selected the coarsest level of the cycle, in place of its `coarse` sweeps,
    1. splits f and the incoming u into the level-0 vectors of an auxiliary hierarchy: a root of the same lengths and per-side
       boundary kinds, log2(n / s) uniform refinements, patch size s;
    2. runs the cycle on it `cycles` times, u carried, with the caller's options (`coarse` now counts sweeps on the one s^D patch);
    3. merges u back.
The auxiliary level-0 beta and sigma are the split of the coarsest level's: a patch's lo block is the matching block of the big lo,
its hi the big lo plane at offset + s, or the big hi on the big patch's upper face. Below that they restrict as ever.

    Sub           the auxiliary hierarchy of a one-patch level: levels, the cell offsets of its level-0 patches, split / merge, and
                  solve: cycle_util.visit on it with u CARRIED (varcoef_util.cycle starts level 0 from zero)
    make_sub      the Sub of a hierarchy's coarsest level; varcoef_util.cycle / bicgstab take it as `sub=` and hand the coarsest
                  level to its solve in place of the sweeps

sigma = None means no reaction term: varcoef_util's functions without sigma, which are those with sigma = 0 bit for bit
(tests/test_reaction_host.py)."""
import numpy as np

from oracle import oracle as orc
from tests import cycle_util, reaction_util as ru, util, varcoef_util as vc


def valid_sub_n(dim, n, s):
    q = n // s if s else 0
    return s >= 4 and s % 2 == 0 and (dim == 2 or s in (4, 8, 16)) and n % s == 0 and q >= 2 and q & (q - 1) == 0


def auto_sub_n(dim, n):
    """sub_n = 0: in 3D 8 where valid (the measured choice), else the smallest valid size (4 where 4 is valid);
    None when there is none"""
    if dim == 3 and valid_sub_n(dim, n, 8):
        return 8
    return next((s for s in range(4, n // 2 + 1, 2) if valid_sub_n(dim, n, s)), None)


class Sub:
    """the auxiliary hierarchy of the one-patch level `big` (an oracle level with P = 1) for sub-patch size s"""

    def __init__(self, big, s, cycles=2):
        from pressurepoissonsolver_amd import capi
        assert big.P == 1 and valid_sub_n(big.dim, big.n, s)
        D, n = big.dim, big.n
        self.dim, self.n, self.s, self.cycles = D, n, s, cycles
        self.mask = int(big.a["neumann"][0])  # every side of the one patch is physical: its bits are the domain's
        self.mesh = capi.Mesh.uniform(D, (n // s).bit_length() - 1)
        self.H = capi.Hierarchy(self.mesh, s, neumann_sides=self.mask)
        lengths = big.a["h"][0] * n  # the auxiliary root has the big patch's lengths
        self.levels = []
        for L in util.independent_levels(self.mesh, self.H):
            a = L.a
            neu = np.zeros(L.P, np.int32)
            for side in range(2 * D):
                if (self.mask >> side) & 1:
                    neu |= (a["nbr_kind"][:, side] == 0).astype(np.int32) << side
            self.levels.append(orc.Level(D, s, a["id"], a["h"] * lengths[None, :], a["nbr_kind"], a["nbr"], a["nbr_orth"], neu, a["parent"],
                                         a["orth_on_parent"]))
        t = self.H.tables(0)
        # cell offsets (x, y[, z]) of the level-0 patches inside the big patch, from the hierarchy's own starts: no order is assumed
        self.origin = np.rint(t["starts"] / t["lengths"]).astype(int) * s
        assert len(self.levels[-1].a["id"]) == 1 and self.levels[0].P == (n // s) ** D

    def _block(self, q):
        """the numpy slices (z, y, x order) of auxiliary patch q inside the big patch"""
        return tuple(slice(self.origin[q][a], self.origin[q][a] + self.s) for a in reversed(range(self.dim)))

    def split(self, v):
        V = np.asarray(v, np.float64).reshape((self.n,) * self.dim)
        return np.concatenate([V[self._block(q)].ravel() for q in range(len(self.origin))])

    def merge(self, w):
        V = np.zeros((self.n,) * self.dim)
        W = np.asarray(w, np.float64).reshape((len(self.origin),) + (self.s,) * self.dim)
        for q in range(len(self.origin)):
            V[self._block(q)] = W[q]
        return V.ravel()

    def split_faces(self, beta):
        """(lo[1, D, n..n], hi[1, D, n^(D-1)]) of the big patch -> (lo[Q, D, s..s], hi[Q, D, s^(D-1)])"""
        D, n, s = self.dim, self.n, self.s
        lo, hi = beta
        Q = len(self.origin)
        slo, shi = np.zeros((Q, D) + (s,) * D), np.zeros((Q, D) + (s,) * (D - 1))
        for q in range(Q):
            blk = self._block(q)
            for a in range(D):
                ax = D - 1 - a
                slo[q, a] = lo[0, a][blk]
                face = tuple(b for i, b in enumerate(blk) if i != ax)
                top = self.origin[q][a] + s
                shi[q, a] = np.take(lo[0, a], top, axis=ax)[face] if top < n else hi[0, a][face]
        return slo, shi

    def set_coefficient(self, beta, sigma=None):
        """the coarsest level's beta (and sigma) -> the auxiliary hierarchy's, every level"""
        self.betas = vc.restrict_all(self.levels, self.split_faces(beta))
        self.sigmas = None if sigma is None else ru.restrict_all(self.levels, self.split(sigma))

    def solve(self, f, u, prolong, smoother=2, omega=6.0 / 7.0, **kw):
        """`cycles` cycles on the auxiliary hierarchy, u CARRIED (varcoef_util.cycle starts level 0 from zero); kw: cycle_util.visit's"""
        A, smooth = vc.operator(self.levels, self.betas, self.sigmas, smoother, omega)
        fa, ua = self.split(f), self.split(u)
        for _ in range(self.cycles):
            ua = cycle_util.visit(self.levels, 0, fa, ua, A, smooth, prolong, **kw)
        return self.merge(ua)


def make_sub(levels, betas, sigmas, s, cycles=2):
    """the Sub of the hierarchy's coarsest level with that level's coefficient set"""
    sub = Sub(levels[-1], s, cycles)
    sub.set_coefficient(betas[-1], None if sigmas is None else sigmas[-1])
    return sub
