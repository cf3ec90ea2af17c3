"""Test infrastructure of adaptive regridding: the normative Python / numpy statements of te_mesh_adapt's
rule (over the node table of capi.Mesh.nodes(): sets of ids), of te_patch_indicator and of the three kinds of te_vec_regrid -- the
specifications the host code and the device kernels are held to."""
import numpy as np

COPY, REFINE, COARSEN = 0, 1, 2


def adapt_rule(nodes, dim, flags):
    """flags: {leaf id: -1 / 0 / +1}. -> dict(R = the refinement set in the order it is applied, families = the coarsened parents
    ascending, new = {refined id: its children's new ids in orthant order}, leaves = the resulting leaf ids ascending)"""
    ilp, nbr, child = nodes["ilp"], nodes["nbr"], nodes["child"]
    row = {int(i): k for k, i in enumerate(ilp[:, 0])}
    parent = lambda i: int(ilp[row[i], 2])  # noqa: E731
    is_leaf = lambda i: child[row[i], 0] == -1  # noqa: E731
    kids = lambda i: [int(c) for c in child[row[i]]]  # noqa: E731
    on_side = lambda o, s: ((o >> (s // 2)) & 1) == (s & 1)  # noqa: E731
    R = {i for i, f in flags.items() if f == 1}
    grew = True
    while grew:
        grew = False
        for x in sorted(R):
            p = parent(x)
            if p == -1:
                continue
            o = kids(p).index(x)
            for s in range(2 * dim):
                y = int(nbr[row[p], s])
                if nbr[row[x], s] == -1 and on_side(o, s) and y != -1 and is_leaf(y) and y not in R:
                    R.add(y)
                    grew = True
    quiet = lambda i: is_leaf(i) and i not in R  # noqa: E731
    families = []
    for P in sorted(row):
        if is_leaf(P) or not all(is_leaf(c) and flags.get(c, 0) == -1 and c not in R for c in kids(P)):
            continue
        ok = True
        for s in range(2 * dim):
            Q = int(nbr[row[P], s])
            if Q == -1 or quiet(Q):
                continue
            ok = ok and not is_leaf(Q) and all(quiet(c) for o, c in enumerate(kids(Q)) if on_side(o, s ^ 1))
        if ok:
            families.append(P)

    def depth(i):
        d = 0
        while parent(i) != -1:
            i, d = parent(i), d + 1
        return d
    order = sorted(R, key=lambda i: (depth(i), i))
    nxt, new = int(ilp[:, 0].max()), {}
    for x in order:
        new[x] = list(range(nxt + 1, nxt + 1 + (1 << dim)))
        nxt += 1 << dim
    leaves = {i for i in row if is_leaf(i)} - R
    for P in families:
        leaves -= set(kids(P))
        leaves.add(P)
    for x in order:
        leaves |= set(new[x])
    return dict(R=order, families=families, new=new, leaves=sorted(leaves))


def indicator(u, P, n, dim):
    """per patch: max over the axes a and the cells whose index along a lies in 1 .. n-2 of |(u[c - e_a] + u[c + e_a]) - 2 u[c]|"""
    v = np.asarray(u).reshape((P,) + (n,) * dim)
    out = np.zeros(P)
    for ax in range(1, dim + 1):
        w = np.moveaxis(v, ax, 1)
        d = np.abs((w[:, :-2] + w[:, 2:]) - 2.0 * w[:, 1:-1])
        out = np.maximum(out, d.reshape(P, -1).max(axis=1))
    return out


def refine_patch(e, o):
    """e: a source patch, shape (n,) * dim (numpy axes z, y, x) -> its child in orthant o. The extended block on -1 .. n per axis is
    filled x then y then z by E[-1] = 3 e[0] - 3 e[1] + e[2], E[n] = 3 e[n-1] - 3 e[n-2] + e[n-3] (later axes extrapolate the ghosts of
    earlier ones); then per axis, c = (i + o_a n) >> 1, d = -1 (i even) / +1 (i odd): v <- (30 E[c] + 5 E[c+d] - 3 E[c-d]) / 32"""
    dim, n = e.ndim, e.shape[0]
    E = np.asarray(e, np.float64)
    for a in range(dim):
        E = np.moveaxis(E, dim - 1 - a, 0)
        lo, hi = 3 * E[0] - 3 * E[1] + E[2], 3 * E[-1] - 3 * E[-2] + E[-3]
        E = np.moveaxis(np.concatenate([lo[None], E, hi[None]], 0), 0, dim - 1 - a)
    i = np.arange(n)
    d = np.where(i % 2 == 0, -1, 1)
    v = E
    for a in range(dim):
        c = (i + ((o >> a) & 1) * n) >> 1
        ax = dim - 1 - a
        v = (30 * np.take(v, c + 1, axis=ax) + 5 * np.take(v, c + d + 1, axis=ax) - 3 * np.take(v, c - d + 1, axis=ax)) / 32
    return v


def coarsen_patch(children):
    """children: the 2^dim source patches by orthant, each (n,) * dim -> their parent: AvgRstr.h:95-102, the fine cells summed x,
    then y, then z, each divided by 2^dim first"""
    dim, n = children[0].ndim, children[0].shape[0]
    h = n // 2
    out = np.zeros((n,) * dim)
    for o, c in enumerate(children):
        acc = np.zeros((h,) * dim)
        for k in range(1 << dim):  # k's bit a = the offset along axis a: x fastest
            sl = tuple(slice((k >> (dim - 1 - ax)) & 1, None, 2) for ax in range(dim))
            acc = acc + c[sl] / (1 << dim)
        out[tuple(slice(((o >> (dim - 1 - ax)) & 1) * h, ((o >> (dim - 1 - ax)) & 1) * h + h) for ax in range(dim))] = acc
    return out


def regrid(src, dst, u_src, n, dim):
    """src / dst: capi.Hierarchy.leaf_tree() of the two hierarchies -> (u_dst, kind per destination patch)"""
    us = np.asarray(u_src).reshape((len(src["id"]),) + (n,) * dim)
    leaf = {int(i): p for p, i in enumerate(src["id"])}
    out, kinds = np.zeros((len(dst["id"]),) + (n,) * dim), []
    for p, (i, par, o) in enumerate(zip(dst["id"], dst["tree_parent"], dst["orthant"])):
        if int(i) in leaf:
            out[p] = us[leaf[int(i)]]
            kinds.append(COPY)
        elif int(par) in leaf:
            out[p] = refine_patch(us[leaf[int(par)]], int(o))
            kinds.append(REFINE)
        else:
            ch = {int(src["orthant"][q]): q for q in np.flatnonzero(src["tree_parent"] == i)}
            assert sorted(ch) == list(range(1 << dim)), f"destination leaf {i} has no source"
            out[p] = coarsen_patch([us[ch[k]] for k in range(1 << dim)])
            kinds.append(COARSEN)
    return out.ravel(), np.array(kinds)


def random_flags(mesh, seed):
    rng = np.random.default_rng(seed)
    return {int(i): int(f) for i, f in zip(mesh.leaves(), rng.integers(-1, 2, len(mesh.leaves())))}


def mixed_flags(mesh):
    """+1 on the family of the leaf nearest the lowest corner, -1 on the family of the leaf nearest the opposite corner that has
    another parent (a family = the leaves among one parent's children)"""
    nd = mesh.nodes()
    leaf = np.flatnonzero(nd["child"][:, 0] == -1)
    leaf = leaf[np.argsort(nd["starts"][leaf].sum(axis=1), kind="stable")]
    ids, par = nd["ilp"][:, 0], nd["ilp"][:, 2]
    lo = par[leaf[0]]
    hi = next(par[k] for k in leaf[::-1] if par[k] != lo)
    fl = {int(ids[k]): 1 for k in leaf if par[k] == lo}
    fl.update({int(ids[k]): -1 for k in leaf if par[k] == hi})
    return fl
