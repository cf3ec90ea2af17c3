"""Tooling: what the reaction term (te_gmg_set_reaction) costs on the device, beside the beta-only kernels and
the constant-coefficient te_apply of the same run. The method of tools/varcoef_time.py: one process; REPS repetitions after a warm-up
round, the operations ALTERNATING inside a repetition (constant coefficient, beta only, beta and sigma). Kernel times from the
library's profile rows (HIP events around each launch), read and reset after each group because the two coefficient groups share
their row names; te_gmg_set_reaction, a cycle and a solve between two HIP events on the solver's stream (medians of REPS). Yardstick:
budget = 1.25 x (algorithmic bytes per site / te_apply's) x the constant-coefficient te_apply's time of the same run.

    python tools/reaction_time.py [--out PATH] [cases ...]       cases as tools/varcoef_time.py: 512, 2refine, 4096; default: all three
Appends one JSON line per case to profiles/reaction_time.jsonl."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402
from tools.varcoef_time import CASES, REPS, ROOT, bytes_per_site, smooth_beta  # noqa: E402

KEYS = ("apply_coef", "resid_coef", "jacobi_coef", "rbgs_coef")


def run(case):
    name, div, n, dim = CASES[case]
    m = capi.Mesh.unit_root(dim) if name == "uniform" else capi.Mesh.read(os.path.join(ROOT, "tests", "golden", name), dim)
    for _ in range(div):
        m.refine_leaves()
    H = capi.Hierarchy(m, n)
    g = capi.GMG(H)
    u, f, out, sigma = g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.init_problem(u, None, problem=capi.PROBLEM_RANDOM)
    g.init_problem(f, None, problem=capi.PROBLEM_RANDOM)
    sigma.set(100.0)
    beta = g.new_face_vector(0, smooth_beta(H, n, dim))
    sites = H.cells(0)
    import torch
    stream = torch.cuda.ExternalStream(g.stream())

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        r = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), r

    opts = g.default_opts(smoother=capi.SMOOTH_RBGS, fuse=0, exact_coarse=0, coarse_sweeps=64)
    wall = dict(set_reaction=[], cycle_beta=[], cycle_sigma=[])
    acc = dict(const={}, beta={}, sigma={})

    def collect(kind):
        g.sync()
        for k, r in g.profile_rows().items():
            a = acc[kind].setdefault(k, [0, 0.0])
            a[0] += r["calls"]
            a[1] += r["ms"]
        g.profile_reset()

    def four():
        g.apply(u, out)
        g.residual(u, f, out)
        g.smooth(f, out, smoother=capi.SMOOTH_RBGS)
        g.smooth(f, out, smoother=capi.SMOOTH_JACOBI)

    def rep(keep):
        g.set_coefficient(None)
        g.profile(True)
        g.profile_reset()
        g.apply(u, out)
        if keep:
            collect("const")
        g.profile(False)
        g.set_coefficient(beta)
        g.profile(True)
        g.profile_reset()
        four()
        if keep:
            collect("beta")
        g.profile(False)  # (the restriction of sigma and the cycle's launches on the small levels stay out of the kernel rows)
        t = timed(lambda: g.cycle(opts, f, out))[0]
        if keep:
            wall["cycle_beta"].append(t)
        t = timed(lambda: g.set_reaction(sigma))[0]
        if keep:
            wall["set_reaction"].append(t)
        g.profile(True)
        g.profile_reset()
        four()
        if keep:
            collect("sigma")
        g.profile(False)
        t = timed(lambda: g.cycle(opts, f, out))[0]
        if keep:
            wall["cycle_sigma"].append(t)

    rep(False)
    for _ in range(REPS):
        rep(True)

    def per_call(rows, key):
        r = rows.get(key)
        return None if not r or not r[0] else r[1] / r[0]

    apply_const = per_call(acc["const"], "stencil_apply") or per_call(acc["const"], "stencil_slabs")
    b_const, b_apply, b_rest = bytes_per_site(n, dim)
    result = dict(tool="tools/reaction_time.py", case=case, mesh=name, divides=div, n=n, dim=dim, sites=sites, reps=REPS,
                  bytes_per_site=dict(apply_const=b_const, apply_coef=b_apply, resid_jacobi_rbgs_coef=b_rest, apply_react=b_apply + 8,
                                      resid_jacobi_rbgs_react=b_rest + 8),
                  apply_const_ms=apply_const, kernels={}, note="level-0 launches only; rbgs_coef: one sweep")
    for key in KEYS:
        b = b_apply if key == "apply_coef" else b_rest
        tb, ts = per_call(acc["beta"], key), per_call(acc["sigma"], key)
        if not tb or not ts or not apply_const:
            continue
        budget = 1.25 * ((b + 8) / b_const) * apply_const
        result["kernels"][key] = dict(beta_ms=round(tb, 4), sigma_ms=round(ts, 4), sigma_over_beta=round(ts / tb, 3), byte_ratio=round((b + 8) / b, 3),
                                      budget_ms=round(budget, 4), fraction_of_budget=round(ts / budget, 3),
                                      tb_per_s=round((b + 8) * sites / (ts * 1e-3) / 1e12, 3))
    for k, v in wall.items():
        result[k + "_ms"] = round(float(np.median(v)), 4)
    # a solve to 1e-10: beta only, then with sigma = 100
    result["solves"] = {}
    o = g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=64)
    x = g.new_vector(0)
    for kind in ("beta", "sigma"):
        g.set_coefficient(beta)
        if kind == "sigma":
            g.set_reaction(sigma)
        g.bicgstab(x, f, o, tol=1e-10, max_it=60)  # warm-up (allocates the work vectors)
        ms = []
        for _ in range(REPS):
            x.set(0.0)
            t, (its, rr) = timed(lambda: g.bicgstab(x, f, o, tol=1e-10, max_it=60))
            ms.append(t)
        result["solves"][kind] = dict(iterations=its, rel_resid=rr, ms=round(float(np.median(ms)), 3), reps=REPS)
    print(json.dumps(result), flush=True)
    return result


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "reaction_time.jsonl")
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
