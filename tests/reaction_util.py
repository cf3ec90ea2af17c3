"""The numpy statement of the reaction term: A_bs u = div(beta grad u) - sigma u (include/te_hip.h te_gmg_set_reaction, DESIGN.md
section 19), the specification the device kernels are held to. The operator, its sweeps, the cycle and BiCGStab are
tests/varcoef_util.py's with `sigma=` / `sigmas=` given; this module holds what is sigma's own.

sigma of a level is a cell vector in the level's layout (L.size doubles), every entry >= 0; beta as in varcoef_util.

    restrict_all     level l + 1's sigma = orc.restrict (te_restrict's average) of level l's; copy-through patches bit for bit
    sigma_from       a function of the coordinates at the cell centres
    manufactured..   the problems of the tests

With sigma = 0 varcoef_util's functions return the bits they return without sigma (tests/test_reaction_host.py)."""
import numpy as np

from oracle import oracle as orc
from tests import varcoef_util as vc


def restrict_all(levels, sigma0):
    sigmas = [np.ascontiguousarray(sigma0, np.float64)]
    for l in range(len(levels) - 1):
        sigmas.append(orc.restrict(levels[l], levels[l + 1], sigmas[-1]))
    return sigmas


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
    beta, u, F0 = vc.manufactured3d()
    sigma = lambda x, y, z: 1.0 + x * x + y * y + z * z
    F = lambda x, y, z: F0(x, y, z) - sigma(x, y, z) * u(x, y, z)
    return beta, sigma, u, F


def manufactured_problem(H, levels, n, dim, beta_fn, sigma_fn, u_fn, F_fn):
    """-> (betas, sigmas per level, right-hand side with the boundary terms of section 18's recipe (1) -- unchanged, sigma multiplies no
    ghost --, exact solution at the cell centres)"""
    betas, rhs, exact = vc.manufactured_problem(H, levels, n, dim, beta_fn, u_fn, F_fn)
    return betas, restrict_all(levels, sigma_from(H.tables(0), n, dim, sigma_fn)), rhs, exact


# ---- what the tests with sigma share
def random_sigma(size, seed):
    """a spread this wide makes a sigma read at the wrong cell or plane show"""
    return np.random.default_rng(seed).uniform(0.0, 50.0, size)


def device_sigmas(g, levels):
    """the solver's sigma on every level, downloaded"""
    out = []
    for l in range(len(levels)):
        v = g.new_vector(l)
        g.reaction(l, v)
        out.append(v.download())
    return out
