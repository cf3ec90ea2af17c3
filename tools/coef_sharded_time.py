"""Tooling: what the variable-coefficient path costs on a SHARDED hierarchy, in loop-back on ONE card: two
virtual ranks (dist.LocalFabric: one thread per rank, exchanges as device-to-device copies with a host rendezvous) share the GPU at
256^3 in 32^3 patches, default placement of the small levels. Per rank, between two HIP events on that rank's solver stream: one
te_gmg_set_coefficient and one V(1,1) RB-GS cycle with the coefficient set; beside them the same two calls of a single-rank solver in
the same process. An equal-bits check comes first (the coefficient on every level and the cycle's result against single rank).

This PRICES the pack kernel, the exchange of the beta blocks and the extra launches of a sharded run. It is NOT a multi-GPU speed-up:
both ranks' kernels run on the one card, one after the other where they do not fit beside each other, and every exchange waits for
the host. There is no pass / fail threshold.

    python tools/coef_sharded_time.py [--out PATH]
Prints one JSON line and appends it to profiles/coef_sharded_time.jsonl."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi, dist as tedist  # noqa: E402
from varcoef_time import smooth_beta  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM, NRANKS = 10, 2, 2
DIVIDES, N, DIM = 3, 32, 3  # 256^3 in 512 patches of 32^3


def timer(g):
    import torch
    stream = torch.cuda.ExternalStream(g.stream())

    def timed(fn):
        """milliseconds between two HIP events on the solver's stream around fn()"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)
    return timed


def measure(g, beta, f, u, opts):
    """-> medians (ms) of te_gmg_set_coefficient and of one cycle; collective on a sharded solver (every rank the same call sequence)"""
    timed = timer(g)
    t_set, t_cyc = [], []
    for i in range(WARM + REPS):
        a = timed(lambda: g.set_coefficient(beta))
        b = timed(lambda: g.cycle(opts, f, u))
        if i >= WARM:
            t_set.append(a)
            t_cyc.append(b)
    return float(np.median(t_set)), float(np.median(t_cyc))


def levels_of(g, H, FV):
    out = []
    for l in range(H.num_levels):
        v = g.new_face_vector(l)
        g.coefficient(l, v)
        out.append(v.download() if v.size else np.empty(0))
    return out


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "coef_sharded_time.jsonl")
    if args and args[0] == "--out":
        path = os.path.abspath(args[1])
    m = capi.Mesh.unit_root(DIM)
    for _ in range(DIVIDES):
        m.refine_leaves()
    nc, FV = N ** DIM, capi.face_vector_size(N, DIM)
    H1 = capi.Hierarchy(m, N)
    g1 = capi.GMG(H1)
    P = H1.sizes(0)[1]
    beta0 = smooth_beta(H1, N, DIM)
    f0 = np.random.default_rng(3).uniform(-1, 1, P * nc)
    opts1 = g1.default_opts(smoother=capi.SMOOTH_RBGS)
    b1, f1, u1 = g1.new_face_vector(0, beta0), g1.new_vector(0, f0), g1.new_vector(0)
    g1.set_coefficient(b1)
    g1.cycle(opts1, f1, u1)
    want_u, want_b = u1.download(), levels_of(g1, H1, FV)

    fab = tedist.LocalFabric(NRANKS)
    hs = [capi.Hierarchy(m, N, rank=r, nranks=NRANKS) for r in range(NRANKS)]
    gs = [capi.GMG(h) for h in hs]
    for r, g in enumerate(gs):
        fab.attach(g, r)

    def body(r):
        H, g = hs[r], gs[r]
        idx = H.l2g(0)
        beta, f, u = g.new_face_vector(0, beta0.reshape(P, FV)[idx]), g.new_vector(0, f0.reshape(P, nc)[idx]), g.new_vector(0)
        opts = g.default_opts(smoother=capi.SMOOTH_RBGS)
        g.set_coefficient(beta)
        g.cycle(opts, f, u)
        same = np.array_equal(u.download(), want_u.reshape(P, nc)[idx].ravel())
        for l, b in enumerate(levels_of(g, H, FV)):
            same = same and np.array_equal(b, want_b[l].reshape(-1, FV)[H.l2g(l)].ravel())
        t_set, t_cyc = measure(g, beta, f, u, opts)
        return dict(rank=r, equal_bits=bool(same), patches=[H.sizes(l)[0] for l in range(H.num_levels)], set_coefficient_ms=round(t_set, 4), cycle_ms=round(t_cyc, 4))

    ranks = fab.run(body)
    if not all(x["equal_bits"] for x in ranks):
        print(json.dumps(dict(tool="tools/coef_sharded_time.py", error="the sharded run does not equal single rank bit for bit", ranks=ranks)), flush=True)
        return 1
    s_set, s_cyc = measure(g1, b1, f1, u1, opts1)  # after the sharded run: the card to itself, as the ranks had it between them
    result = dict(tool="tools/coef_sharded_time.py", mesh="uniform", divides=DIVIDES, n=N, dim=DIM, sites=P * nc, nranks=NRANKS, reps=REPS,
                  equal_bits=True, single_rank=dict(set_coefficient_ms=round(s_set, 4), cycle_ms=round(s_cyc, 4)), ranks=ranks,
                  note="two virtual ranks in loop-back on ONE card (host rendezvous per exchange): the price of pack, exchange and extra launches, "
                       "not a multi-GPU speed-up; one run")
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as fh:
        fh.write(json.dumps(result) + "\n")
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
