"""Tooling: what the full-multigrid solve te_fmg costs next to te_bicgstab, and what it delivers. The trig problem (Dirichlet, exact
face data) on uniform 256^3 and 512^3 in 32^3 patches, the linear interpolator, V(1,1) with RB-GS and with the reference smoother:
te_fmg with cycles = 1 and 2 (ms, error against the analytic solution, relative residual) beside te_bicgstab to 1e-12 from zero (ms,
iterations, error), alternating in one process, event times on the solver's stream over REPS repetitions after a warm-up round.
Then the level-0 kernels side by side from the library's profile rows in the same run: k_prolong_quadratic3d, k_prolong3d
(te_prolong_add), k_prolong_linear3d and te_apply, the quadratic kernel's time as a fraction of the budget
1.25 x (its bytes / te_apply's bytes) x te_apply's time. Writes profiles/fmg_solve.json.

    python tools/fmg_solve.py [--out PATH] [sizes ...]        (default: 256 512)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
SMOOTHERS = (("rbgs", capi.SMOOTH_RBGS), ("patch_solve", capi.SMOOTH_PATCH_SOLVE))
N = 32
# algorithmic bytes per level-0 site: one value per cell plus the six halo layers of a patch (te_apply reads u and writes f; the
# quadratic interpolation writes fine and reads 1/8 of a coarse value plus the ring of the parent's octant; the two corrections
# read and write fine)
HALO = 6.0 / N * 8
BYTES = dict(stencil_apply=16 + HALO, prolong_quadratic=8 + 1 + 6 * 16 ** 2 / N ** 3 * 8, prolong_linear=16 + 1 + 6 * 16 ** 2 / N ** 3 * 8, prolong_add=17.0)


def event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def run(size):
    H = capi.Hierarchy(capi.Mesh.uniform(3, int(round(np.log2(size // N)))), N)
    g = capi.GMG(H)
    stream = torch.cuda.ExternalStream(g.stream())
    F, exact, f, x, tmp = (g.new_vector(0) for _ in range(5))
    bd = g.new_boundary_vector(0)
    g.init_problem(F, exact, problem=capi.PROBLEM_TRIG)      # the folded right-hand side te_bicgstab solves
    g.boundary_sample(bd, problem=capi.PROBLEM_TRIG)
    f.copy(F)
    g.add_boundary_rhs(g.new_boundary_vector(0, -bd.download()), f)  # the interior right-hand side te_fmg takes (the fold is linear in the data)
    enorm = exact.twoNorm()

    def error():
        tmp.copy(x)
        tmp.addScaled(-1.0, exact)
        return tmp.twoNorm() / enorm

    g.set_interpolator(capi.INTERP_LINEAR)
    out = dict(size=size, n=N, patches=H.sizes(0)[1], levels=H.num_levels, reps=REPS, solve={})
    for sname, sm in SMOOTHERS:
        o = g.default_opts(smoother=sm)

        def solve():
            x.set(0.0)
            return g.bicgstab(x, F, o)
        calls = dict(fmg1=lambda: g.fmg(f, x, o, bdata=bd, cycles=1), fmg2=lambda: g.fmg(f, x, o, bdata=bd, cycles=2), bicgstab=solve)
        res = {k: dict(ms=[]) for k in calls}
        for rep in range(REPS + 1):  # alternating; the first round warms up (work vectors, code objects)
            for k, fn in calls.items():
                ms, ret = event_ms(stream, fn)
                if rep:
                    res[k]["ms"].append(round(ms, 3))
                if rep == REPS:
                    res[k]["error_vs_analytic"] = error()
                    if k == "bicgstab":
                        res[k]["iterations"], res[k]["rel_resid"] = ret
                    else:
                        res[k]["rel_resid"] = ret
        for k in res:
            res[k]["ms_min"], res[k]["ms_median"] = min(res[k]["ms"]), float(np.median(res[k]["ms"]))
        out["solve"][sname] = res
        print(f"{size}^3 {sname}: " + "; ".join(f"{k}: {v['ms_median']:.2f} ms (min {v['ms_min']:.2f}), error {v['error_vs_analytic']:.3e}"
                                                + (f", {v['iterations']} its" if "iterations" in v else "") for k, v in res.items()), flush=True)
    g.set_interpolator(capi.INTERP_DIRECT)
    g.release_workspace()
    # the level-0 kernels, same vectors, alternating
    e = g.new_vector(1)
    g.init_problem(e, None, problem=capi.PROBLEM_RANDOM, level=1)
    ops = dict(stencil_apply=lambda: g.apply(x, tmp), prolong_quadratic=lambda: g.interpolate_quadratic(e, x, fine_level=0),
               prolong_add=lambda: g.interpolate(e, x, fine_level=0), prolong_linear=lambda: g.interpolate_linear(e, x, fine_level=0))
    for _ in range(3):
        for fn in ops.values():
            fn()
    g.sync()
    g.profile(True)
    g.profile_reset()
    for _ in range(REPS):
        for fn in ops.values():
            fn()
    rows = g.profile_rows()
    g.profile(False)
    ms = {k: rows[k]["ms"] / rows[k]["calls"] for k in ops}
    out["level0_kernels"] = dict(ms={k: round(v, 4) for k, v in ms.items()}, bytes_per_site={k: round(v, 3) for k, v in BYTES.items()},
                                 tb_per_s={k: round(BYTES[k] * H.cells(0) / (ms[k] * 1e-3) / 1e12, 3) for k in ops},
                                 quadratic_ratio_to_budget=round(ms["prolong_quadratic"] / (1.25 * BYTES["prolong_quadratic"] / BYTES["stencil_apply"] * ms["stencil_apply"]), 3))
    print(f"{size}^3 level-0 kernels: {out['level0_kernels']}", flush=True)
    return out


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "fmg_solve.json")
    if args and args[0] == "--out":
        path, args = os.path.abspath(args[1]), args[2:]
    sizes = [int(a) for a in args] or [256, 512]
    result = dict(tool="tools/fmg_solve.py", problem="trig, Dirichlet, exact face data, V(1,1), linear interpolator, uniform, 32^3 patches; te_bicgstab to 1e-12",
                  runs=[run(s) for s in sizes])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
