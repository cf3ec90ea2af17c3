"""CPU: the numpy statement of te_faces_regrid (tests/faceregrid_util.py) on its own, n = 4 and 8, 2D and 3D, cubic spacing and the
stretched h = (1, 0.7, 1.3) / n.

Bounds. Divergence: a fine cell's divergence differs from its coarse cell's by at most 64 eps sum_a max|U_a| / h_a^fine -- two face
values per axis, each the result of at most 6 roundings of partial results no larger than 4 max|U|, give 48; 64 leaves a margin, and a
wrong weight is off by O(0.1 max|U| / h). Linear fields: 64 eps max|U|. A smooth field: second order, the error falls by 3.5 to 4.5
from n to 2n."""
import numpy as np
import pytest

from tests import faceregrid_util as fu

EPS = np.finfo(np.float64).eps
CASES = [(n, dim, hs) for n in (4, 8) for dim in (2, 3) for hs in ("cubic", "stretched")]


def spacing(n, dim, hs):
    return (np.ones(3) if hs == "cubic" else np.array([1.0, 0.7, 1.3]))[:dim] / n


def random_faces(n, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, [n + (dim - 1 - ax == a) for ax in range(dim)]) for a in range(dim)]


def sample(fn, n, dim, h, origin):
    """fn(a, x) on the face centres of a patch with lower corner `origin` and spacings h; x = [x_0 .. x_{dim-1}] broadcastable"""
    F = []
    for a in range(dim):
        x = []
        for b in range(dim):
            shape = [1] * dim
            shape[dim - 1 - b] = n + (b == a)
            x.append((origin[b] + (np.arange(n + 1) if b == a else np.arange(n) + 0.5) * h[b]).reshape(shape))
        F.append(fn(a, x) + np.zeros([n + (dim - 1 - ax == a) for ax in range(dim)]))
    return F


@pytest.mark.parametrize("n,dim,hs", CASES)
def test_refine_preserves_divergence(n, dim, hs):
    h = spacing(n, dim, hs)
    F = random_faces(n, dim, 1)
    coarse, bound, worst = fu.divergence(F, h), fu.div_bound(F, h / 2), 0.0
    for o in range(1 << dim):
        fine = fu.divergence(fu.refine_faces(F, o, h), h / 2)
        worst = max(worst, np.abs(fine - fu.parent_cells(coarse, o, n, dim)).max())
    print(f"n={n} {dim}D {hs}: defect {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


@pytest.mark.parametrize("n,dim,hs", CASES)
def test_refine_reproduces_linear_fields(n, dim, hs):
    h = spacing(n, dim, hs)
    rng = np.random.default_rng(2)
    c0, c = rng.uniform(-1, 1, dim), rng.uniform(-1, 1, (dim, dim))
    fn = lambda a, x: c0[a] + sum(c[a, b] * x[b] for b in range(dim))  # noqa: E731
    F = sample(fn, n, dim, h, np.zeros(dim))
    M = max(np.abs(f).max() for f in F)
    for o in range(1 << dim):
        want = sample(fn, n, dim, h / 2, [((o >> b) & 1) * n * h[b] / 2 for b in range(dim)])
        got = fu.refine_faces(F, o, h)
        err = max(np.abs(g - w).max() for g, w in zip(got, want))
        assert err <= 64 * EPS * M, (o, err)


@pytest.mark.parametrize("n,dim,hs", CASES)
def test_refine_is_second_order(n, dim, hs):
    fn = lambda a, x: np.sin(1.3 * x[0] + 0.4 * a) * np.cos(0.9 * x[1] - 0.2 * a) * (np.sin(1.1 * x[2] + 0.3) if dim == 3 else 1.0)  # noqa: E731
    errs = []
    for m in (n, 2 * n):
        h = spacing(m, dim, hs)
        F, e = sample(fn, m, dim, h, np.zeros(dim)), 0.0
        for o in range(1 << dim):
            want = sample(fn, m, dim, h / 2, [((o >> b) & 1) * m * h[b] / 2 for b in range(dim)])
            e = max(e, max(np.abs(g - w).max() for g, w in zip(fu.refine_faces(F, o, h), want)))
        errs.append(e)
    print(f"n={n} {dim}D {hs}: errors {errs[0]:.3e} -> {errs[1]:.3e}, ratio {errs[0] / errs[1]:.2f}")
    assert 3.5 <= errs[0] / errs[1] <= 4.5


@pytest.mark.parametrize("n,dim,hs", CASES)
def test_coarsen_gives_the_mean_divergence(n, dim, hs):
    hf = spacing(n, dim, hs)  # the children's spacing; the parent's is twice that
    ch = [random_faces(n, dim, 10 + o) for o in range(1 << dim)]
    # the children agree on the faces they share, as a face vector on a mesh does
    for o in range(1 << dim):
        for a in range(dim):
            if (o >> a) & 1:
                lo = np.moveaxis(ch[o ^ (1 << a)][a], dim - 1 - a, 0)
                np.moveaxis(ch[o][a], dim - 1 - a, 0)[0] = lo[n]
    coarse = fu.divergence(fu.coarsen_faces(ch), 2 * hf)
    bound = max(fu.div_bound(c, hf) for c in ch)
    worst = np.abs(coarse - fu.children_mean([fu.divergence(c, hf) for c in ch], dim)).max()
    print(f"n={n} {dim}D {hs}: defect {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


@pytest.mark.parametrize("n,dim,hs", CASES)
def test_shared_faces_of_refined_siblings_are_bit_identical(n, dim, hs):
    h = spacing(n, dim, hs)
    for a in range(dim):
        X, Y = random_faces(n, dim, 20 + a), random_faces(n, dim, 30 + a)  # Y is X's upper neighbour along a
        np.moveaxis(Y[a], dim - 1 - a, 0)[0] = np.moveaxis(X[a], dim - 1 - a, 0)[n]
        for o in range(1 << dim):
            if not (o >> a) & 1:
                continue
            up = np.moveaxis(fu.refine_faces(X, o, h)[a], dim - 1 - a, 0)
            across = np.moveaxis(fu.refine_faces(Y, o ^ (1 << a), h)[a], dim - 1 - a, 0)
            inside = np.moveaxis(fu.refine_faces(X, o ^ (1 << a), h)[a], dim - 1 - a, 0)
            assert np.array_equal(up[n], across[0]), (a, o)  # the children of two adjacent refined patches
            assert np.array_equal(up[0], inside[n]), (a, o)  # two children of one patch


def test_layout_round_trip():
    from pressurepoissonsolver_amd import capi
    for n, dim in ((4, 2), (4, 3)):
        a = np.arange(2 * capi.face_vector_size(n, dim), dtype=np.float64)
        lo, hi = capi.face_vector_views(a, n, dim)
        b = np.zeros_like(a)
        lo2, hi2 = capi.face_vector_views(b, n, dim)
        for p in range(2):
            F = fu.patch_faces(lo[p], hi[p], n, dim)
            assert F[0].shape == (n,) * (dim - 1) + (n + 1,)
            fu.store_faces(F, lo2[p], hi2[p], n, dim)
        assert np.array_equal(a, b)
