"""Tooling: what the variable-coefficient path (te_gmg_set_coefficient) costs on the device, beside the
constant-coefficient kernels of the same run. One process; REPS repetitions after a warm-up round, the operations ALTERNATING inside a
repetition. Kernel times from the library's profile rows (HIP events around each launch); te_gmg_set_coefficient, a cycle and a solve
between two HIP events recorded on the solver's stream (medians of REPS). The yardstick is section 13's: a kernel's budget is 1.25 x (its algorithmic bytes per
site / te_apply's) x the constant-coefficient te_apply's time of the same run.

    python tools/varcoef_time.py [--out PATH] [cases ...]        cases: 512 (512^3, 32^3 patches), 2refine (2refine.bin --divide 3),
                                                                 4096 (2D 4096^2, 64^2 patches); default: all three
Appends one JSON line per case to profiles/varcoef_time.jsonl."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
CASES = {"512": ("uniform", 4, 32, 3), "2refine": ("2refine.bin", 3, 32, 3), "4096": ("uniform", 6, 64, 2)}


def bytes_per_site(n, dim):
    """algorithmic bytes per site: (constant-coefficient apply, A_b apply, A_b residual / Jacobi / RB-GS)"""
    halo = 2 * dim / n * 8  # the face layers read around a patch
    beta = dim * 8 + dim * 8 / n  # the three (two) lower faces of a cell and its share of the HI blocks
    return 16 + halo, 8 + halo + beta + 8, 8 + halo + beta + 16


def smooth_beta(H, n, dim):
    """1 + 0.5 prod_i sin(2 pi (x_i + 0.1 i)) at the face centres, as a flat face vector"""
    t = H.tables(0)
    P = len(t["id"])
    nc, nf = n ** dim, n ** (dim - 1)
    out = np.empty((P, dim * nc + dim * nf))
    idx = np.indices((n,) * dim)[::-1].reshape(dim, -1)  # row a = index along axis a, x fastest
    fidx = np.indices((n,) * (dim - 1))[::-1].reshape(dim - 1, -1)
    fn = lambda x: 1.0 + 0.5 * np.prod([np.sin(2 * np.pi * (x[i] + 0.1 * i)) for i in range(dim)], axis=0)
    for p in range(P):
        h = t["lengths"][p] / n
        for a in range(dim):
            x = [t["starts"][p][b] + (idx[b] + (0.0 if b == a else 0.5)) * h[b] for b in range(dim)]
            out[p, a * nc:(a + 1) * nc] = fn(x)
            others = [b for b in range(dim) if b != a]
            x = [None] * dim
            x[a] = np.full(nf, t["starts"][p][a] + t["lengths"][p][a])
            for k, b in enumerate(others):
                x[b] = t["starts"][p][b] + (fidx[k] + 0.5) * h[b]
            out[p, dim * nc + a * nf:dim * nc + (a + 1) * nf] = fn(x)
    return out.ravel()


def run(case):
    name, div, n, dim = CASES[case]
    m = capi.Mesh.unit_root(dim) if name == "uniform" else capi.Mesh.read(os.path.join(ROOT, "tests", "golden", name), dim)
    for _ in range(div):
        m.refine_leaves()
    H = capi.Hierarchy(m, n)
    g = capi.GMG(H)
    u, f, out = g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.init_problem(u, None, problem=capi.PROBLEM_RANDOM)
    g.init_problem(f, None, problem=capi.PROBLEM_RANDOM)
    beta = g.new_face_vector(0, smooth_beta(H, n, dim))
    sites = H.cells(0)
    import torch
    stream = torch.cuda.ExternalStream(g.stream())

    def timed(fn):
        """milliseconds between two HIP events on the solver's stream around fn()"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        r = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), r

    opts = g.default_opts(smoother=capi.SMOOTH_RBGS, fuse=0, exact_coarse=0, coarse_sweeps=64)

    def const_ops():
        g.set_coefficient(None)
        g.apply(u, out)
        g.smooth(f, out, smoother=capi.SMOOTH_RBGS)

    def coef_ops(wall):
        wall["set_coefficient"].append(timed(lambda: g.set_coefficient(beta))[0])
        g.apply(u, out)
        g.residual(u, f, out)
        g.smooth(f, out, smoother=capi.SMOOTH_RBGS)
        g.smooth(f, out, smoother=capi.SMOOTH_JACOBI)
        g.sync()
        g.profile(False)  # (the cycle's launches on the small levels stay out of the kernel rows)
        wall["cycle"].append(timed(lambda: g.cycle(opts, f, out))[0])
        g.profile(True)

    wall = dict(set_coefficient=[], cycle=[])
    const_ops()
    coef_ops(dict(set_coefficient=[], cycle=[]))
    g.sync()
    g.profile(True)
    g.profile_reset()
    for _ in range(REPS):  # the constant-coefficient rows and the coefficient rows are kept apart: a cycle launches coefficient kernels only
        const_ops()
    rows_const = g.profile_rows()
    g.profile_reset()
    for _ in range(REPS):
        const_ops()
        g.profile(False)
        g.sync()
        g.profile(True)
        coef_ops(wall)
    rows_coef = g.profile_rows()
    g.profile(False)

    def per_call(rows, key):
        r = rows.get(key)
        return None if not r or not r["calls"] else r["ms"] / r["calls"]

    apply_const = per_call(rows_const, "stencil_apply") or per_call(rows_const, "stencil_slabs")
    rbgs_const = per_call(rows_const, "stencil_rbgs") or per_call(rows_const, "stencil_rbgs_slabs")
    b_const, b_apply, b_rest = bytes_per_site(n, dim)
    result = dict(tool="tools/varcoef_time.py", case=case, mesh=name, divides=div, n=n, dim=dim, sites=sites, reps=REPS,
                  bytes_per_site=dict(apply_const=b_const, apply_coef=b_apply, resid_jacobi_rbgs_coef=b_rest),
                  apply_const_ms=apply_const, rbgs_const_ms=rbgs_const, kernels={}, note="level-0 launches only (the cycle runs unprofiled); rbgs_coef: one sweep; "
                  "faces_restrict: all levels of one te_gmg_set_coefficient")
    for key, b in (("apply_coef", b_apply), ("resid_coef", b_rest), ("jacobi_coef", b_rest), ("rbgs_coef", b_rest), ("faces_restrict", None)):
        r = rows_coef.get(key)
        if not r or not r["calls"]:
            continue
        ms = r["ms"] / REPS if b is None else r["ms"] / r["calls"]
        k = dict(ms=round(ms, 4), calls=r["calls"])
        if b is not None and apply_const:
            budget = 1.25 * (b / b_const) * apply_const
            k.update(budget_ms=round(budget, 4), fraction_of_budget=round(ms / budget, 3), tb_per_s=round(b * sites / (ms * 1e-3) / 1e12, 3))
        result["kernels"][key] = k
    result["set_coefficient_ms"] = round(float(np.median(wall["set_coefficient"])), 4)
    result["cycle_ms"] = round(float(np.median(wall["cycle"])), 4)
    # a solve to 1e-10 with the smooth coefficient
    g.set_coefficient(beta)
    result["solves"] = {}
    for cs in (64, 256):
        o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=cs)
        x = g.new_vector(0)
        g.bicgstab(x, f, o, tol=1e-10, max_it=60)  # warm-up (allocates the work vectors)
        ms = []
        for _ in range(REPS):
            x.set(0.0)
            t, (its, rr) = timed(lambda: g.bicgstab(x, f, o, tol=1e-10, max_it=60))
            ms.append(t)
        result["solves"][str(cs)] = dict(iterations=its, rel_resid=rr, ms=round(float(np.median(ms)), 3), reps=REPS)
    print(json.dumps(result), flush=True)
    return result


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "varcoef_time.jsonl")
    if args and args[0] == "--out":
        path, args = os.path.abspath(args[1]), args[2:]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    for case in args or list(CASES):
        r = run(case)
        with open(path, "a") as fh:
            fh.write(json.dumps(r) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
