"""Tooling: what the sub-patch coarse solve of the variable-coefficient path (te_gmg_set_coef_coarse) costs on the
device beside plain sweeps on the one-patch coarsest level. The method of tools/reaction_time.py: one process; REPS repetitions after a
warm-up round, the kinds ALTERNATING inside a repetition; every time between two HIP events on the solver's stream (medians of REPS).

Per configuration -- SWEEPS with coarse_sweeps 64 and 256, SUBCYCLE with sub_n in {4, 8, 16 where valid} x cycles in {1, 2} and
coarse_sweeps = 2 sub_n --
    coarse_ms   the coarse solve ALONE: te_vcycle of a one-level solver on the root with patch size n that holds the big solver's
                coarsest-level beta (its cycle is the coarsest level's work and nothing else), with its launches from the profile rows
                of a separate, untimed cycle (the rows of that solver and of its auxiliary solver)
    cycle_ms    one V(1,1) RB-GS cycle of the whole hierarchy
    solve       te_bicgstab to 1e-10 on section 18's right-hand side: iterations and time
The yardstick is the SWEEPS 64 row of the same run. One run on one box.

    python tools/coef_coarse_time.py [--out PATH] [cases ...]    cases as tools/varcoef_time.py: 512, 2refine, 4096; default: all three
Appends one JSON line per case to profiles/coef_coarse_time.jsonl."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402
from tools.varcoef_time import CASES, REPS, ROOT, smooth_beta  # noqa: E402

SUB, SWEEPS = capi.COEF_COARSE_SUBCYCLE, capi.COEF_COARSE_SWEEPS


def valid(dim, n, s):
    q = n // s
    return n % s == 0 and q >= 2 and q & (q - 1) == 0 and (dim == 2 or s in (4, 8, 16))


def run(case):
    name, div, n, dim = CASES[case]
    m = capi.Mesh.unit_root(dim) if name == "uniform" else capi.Mesh.read(os.path.join(ROOT, "tests", "golden", name), dim)
    for _ in range(div):
        m.refine_leaves()
    H = capi.Hierarchy(m, n)
    g = capi.GMG(H)
    lc = g.num_levels - 1
    assert H.sizes(lc)[1] == 1
    f, out, x = g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.init_problem(f, None, problem=capi.PROBLEM_RANDOM)
    g.set_coefficient(g.new_face_vector(0, smooth_beta(H, n, dim)))
    # the coarse solve alone: the root as ONE patch of n^dim with the coarsest level's beta
    H1 = capi.Hierarchy(capi.Mesh.unit_root(dim), n)
    g1 = capi.GMG(H1)
    bc = g.new_face_vector(lc)
    g.coefficient(lc, bc)
    g1.set_coefficient(g1.new_face_vector(0, bc.download()))
    f1, u1 = g1.new_vector(0), g1.new_vector(0)
    g1.init_problem(f1, None, problem=capi.PROBLEM_RANDOM)
    import torch

    def timed(s, fn):
        st = torch.cuda.ExternalStream(s.stream())
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        r = fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b), r

    configs = [("sweeps", 0, 1, 64), ("sweeps", 0, 1, 256)]
    configs += [("subcycle", s, c, 2 * s) for s in (4, 8, 16) if valid(dim, n, s) for c in (1, 2)]
    label = lambda k: f"{k[0]}_{k[3]}" if k[0] == "sweeps" else f"sub{k[1]}_x{k[2]}_{k[3]}"
    acc = {label(k): dict(coarse=[], cycle=[], solve=[], its=None, rr=None) for k in configs}

    def select(k):
        for s in (g, g1):
            s.set_coef_coarse(SWEEPS if k[0] == "sweeps" else SUB, k[1], k[2])
        return g.default_opts(smoother=capi.SMOOTH_RBGS, coarse_sweeps=k[3])

    def rep(keep):
        for k in configs:
            o = select(k)
            a = acc[label(k)]
            t = timed(g1, lambda: g1.cycle(o, f1, u1))[0]
            keep and a["coarse"].append(t)
            t = timed(g, lambda: g.cycle(o, f, out))[0]
            keep and a["cycle"].append(t)
            x.set(0.0)
            t, (its, rr) = timed(g, lambda: g.bicgstab(x, f, o, tol=1e-10, max_it=60))
            keep and a["solve"].append(t)
            a["its"], a["rr"] = its, rr

    rep(False)
    for _ in range(REPS):
        rep(True)
    result = dict(tool="tools/coef_coarse_time.py", case=case, mesh=name, divides=div, n=n, dim=dim, sites=H.cells(0), levels=g.num_levels, reps=REPS,
                  note="coarse_ms: te_vcycle of a one-level solver on the root (one patch of n^dim) with the coarsest level's beta", configs={})
    base = None
    for k in configs:
        o = select(k)
        g1.profile(True)
        g1.profile_reset()
        g1.cycle(o, f1, u1)
        rows = g1.profile_rows()
        g1.profile(False)
        a = acc[label(k)]
        r = dict(kind=k[0], sub_n=g1.coef_coarse()[1] if k[0] != "sweeps" else 0, cycles=k[2], coarse_sweeps=k[3],
                 coarse_ms=round(float(np.median(a["coarse"])), 4), cycle_ms=round(float(np.median(a["cycle"])), 4),
                 solve_ms=round(float(np.median(a["solve"])), 3), iterations=a["its"], rel_resid=a["rr"],
                 coarse_launches=int(sum(v["calls"] for v in rows.values())),
                 coarse_rows={kk: dict(calls=int(v["calls"]), ms=round(v["ms"], 4)) for kk, v in rows.items()})
        base = base or r
        r["over_sweeps_64"] = dict(coarse=round(r["coarse_ms"] / base["coarse_ms"], 3), cycle=round(r["cycle_ms"] / base["cycle_ms"], 3),
                                   solve=round(r["solve_ms"] / base["solve_ms"], 3))
        result["configs"][label(k)] = r
    for s in (g, g1):
        s.set_coef_coarse(SWEEPS)
    print(json.dumps(result), flush=True)
    return result


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "coef_coarse_time.jsonl")
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
