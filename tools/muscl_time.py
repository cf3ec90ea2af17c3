"""Tooling: what the second-order transport calls (te_cell_slopes, te_advect_flux_muscl, te_advect_muscl) cost on
the device at 512^3, beside te_advect of the same run as the yardstick and the four-call composition te_advect_muscl replaces
(te_advect_flux_muscl -> te_divergence -> te_vec_copy + te_vec_add_scaled). One process; REPS repetitions after a warm-up round, the
operations ALTERNATING inside a repetition, each between two HIP events recorded on the solver's stream (medians of REPS, as
tools/advect_time.py takes them); the kernels' own times from the library's profile rows as well. A call's budget is its algorithmic
bytes per site (csrc/musclkernels.hpp) at 8 TB/s.

    python tools/muscl_time.py [--out PATH] [cases ...]    cases: 512 (512^3, 32^3 patches), 2refine (2refine.bin --divide 3),
                                                           4096 (2D 4096^2, 64^2 patches); default: 512
Appends one JSON line per case to profiles/muscl_time.jsonl."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
PEAK = 8e12  # B/s
CASES = {"512": ("uniform", 4, 32, 3), "2refine": ("2refine.bin", 3, 32, 3), "4096": ("uniform", 6, 64, 2)}
KIND = capi.SLOPE_MC


def bytes_per_site(n, dim):
    """algorithmic bytes per site of each call (the two marches' entry points run the slope pass first)"""
    halo = 2 * dim / n * 8  # the face layers read around a patch
    face = dim * 8 + dim * 8 / n  # the lower faces of a cell and its share of the HI blocks
    slopes = 8 + halo + dim * 8
    sread = dim * (8 + 2 / n * 8)  # each slope vector with the two facing layers along its axis
    flux = slopes + 8 + halo + face + sread + face
    fused = slopes + 8 + halo + face + sread + 8
    return dict(cell_slopes=slopes, advect_flux_muscl=flux, advect_muscl=fused, advect=8 + halo + face + 8, composition=flux + (face + 8) + 16 + 24)


def run(case):
    name, div, n, dim = CASES[case]
    m = capi.Mesh.unit_root(dim) if name == "uniform" else capi.Mesh.read(os.path.join(ROOT, "tests", "golden", name), dim)
    for _ in range(div):
        m.refine_leaves()
    H = capi.Hierarchy(m, n)
    g = capi.GMG(H)
    sites = H.cells(0)
    p, c, out, d = g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0)
    S = [g.new_vector(0) for _ in range(dim)]
    g.init_problem(p, None, problem=capi.PROBLEM_RANDOM)
    c.set(2.0)
    c.addScaled(0.5, p)  # a positive cell field in [1.5, 2.5]
    U, F = g.new_face_vector(0), g.new_face_vector(0)
    g.gradient(p, U)  # a face field with both signs
    alpha = 0.5 / (2 * dim * g.faces_max_rate(U))
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

    def composition():
        g.advect_flux_muscl(U, c, F, kind=KIND)
        g.divergence(F, d, alpha=alpha)
        out.copy(c)
        out.addScaled(-1.0, d)

    ops = dict(cell_slopes=lambda: g.cell_slopes(c, S[0], S[1], S[2] if dim == 3 else None, kind=KIND),
               advect_flux_muscl=lambda: g.advect_flux_muscl(U, c, F, kind=KIND), advect_muscl=lambda: g.advect_muscl(U, c, out, alpha=alpha, kind=KIND),
               advect=lambda: g.advect(U, c, out, alpha=alpha), composition=composition)
    wall = {k: [] for k in ops}

    def rep(keep):
        for k, fn in ops.items():
            g.profile(k != "composition")  # (the composition's launches stay out of the kernel rows: they would be counted twice)
            t = timed(fn)
            if keep:
                wall[k].append(t)
        g.profile(True)

    g.profile(True)
    rep(False)
    g.sync()
    g.profile_reset()
    for _ in range(REPS):
        rep(True)
    rows = g.profile_rows()
    g.profile(False)
    b = bytes_per_site(n, dim)
    result = dict(tool="tools/muscl_time.py", case=case, mesh=name, divides=div, n=n, dim=dim, sites=sites, reps=REPS, kind="MC", bytes_per_site=b, ops={},
                  kernels={})
    for k in ops:
        ms = float(np.median(wall[k]))
        result["ops"][k] = dict(ms=round(ms, 4), budget_ms=round(b[k] * sites / PEAK * 1e3, 4), budget_over_time=round(b[k] * sites / PEAK * 1e3 / ms, 3),
                                tb_per_s=round(b[k] * sites / (ms * 1e-3) / 1e12, 3), over_advect=None)
    for k in ops:
        result["ops"][k]["over_advect"] = round(result["ops"][k]["ms"] / result["ops"]["advect"]["ms"], 3)
    for k in ("cell_slopes", "advect_flux_muscl", "advect_muscl", "advect", "cf_ghost"):
        r = rows.get(k)
        if r and r["calls"]:
            result["kernels"][k] = dict(ms=round(r["ms"] / r["calls"], 4), calls=r["calls"])
    result["advect_muscl_over_composition"] = round(result["ops"]["advect_muscl"]["ms"] / result["ops"]["composition"]["ms"], 3)
    # the fraction of peak te_advect_muscl reaches, over the fraction te_advect reaches in the same run
    result["fraction_of_advects_fraction"] = round(result["ops"]["advect_muscl"]["budget_over_time"] / result["ops"]["advect"]["budget_over_time"], 3)
    print(json.dumps(result), flush=True)
    return result


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "muscl_time.jsonl")
    if args and args[0] == "--out":
        path, args = os.path.abspath(args[1]), args[2:]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    for case in args or ["512"]:
        r = run(case)
        with open(path, "a") as fh:
            fh.write(json.dumps(r) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
