"""Tooling: what the three calls of the variable-density step (te_faces_from_cells, te_project_weighted,
te_add_boundary_rhs_weighted) cost on the device, beside what they replace. One process; REPS repetitions after
a warm-up round, the operations ALTERNATING inside a repetition. Kernel times from the library's profile rows (HIP events around each
launch on the solver's stream); the fused projection and the three-call recipe te_gradient -> te_vec_multiply -> te_vec_add_scaled
also between two HIP events recorded on the solver's stream (medians of REPS); the upload of a host-built face vector by the host's
clock around upload + synchronise (median of 5). The yardstick is section 13's: a kernel's budget is 1.25 x (its algorithmic bytes
per site / te_apply's) x the constant-coefficient te_apply's time of the same run.

    python tools/density_step_time.py [--out PATH] [cases ...]   cases: 512 (512^3, 32^3 patches), 2refine (2refine.bin --divide 3),
                                                                 4096 (2D 4096^2, 64^2 patches); default: all three
Appends one JSON line per case to profiles/density_step_time.jsonl."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
CASES = {"512": ("uniform", 4, 32, 3), "2refine": ("2refine.bin", 3, 32, 3), "4096": ("uniform", 6, 64, 2)}


def bytes_per_site(n, dim):
    """algorithmic bytes per site: te_apply, gradient, faces_from_cells, project, project_weighted"""
    halo = 2 * dim / n * 8  # the face layers read around a patch
    face = dim * 8 + dim * 8 / n  # the lower faces of a cell and its share of the HI blocks
    return dict(apply=16 + halo, gradient=8 + halo + face, faces_from_cells=8 + halo + face, project=8 + halo + 2 * face,
                project_weighted=8 + halo + 3 * face)


def run(case):
    name, div, n, dim = CASES[case]
    m = capi.Mesh.unit_root(dim) if name == "uniform" else capi.Mesh.read(os.path.join(ROOT, "tests", "golden", name), dim)
    for _ in range(div):
        m.refine_leaves()
    H = capi.Hierarchy(m, n)
    g = capi.GMG(H)
    sites = H.cells(0)
    p, c, out, f = g.new_vector(0), g.new_vector(0), g.new_vector(0), g.new_vector(0)
    g.init_problem(p, None, problem=capi.PROBLEM_RANDOM)
    c.set(2.0)
    c.addScaled(0.5, p)  # a positive cell field in [1.5, 2.5]
    F, U, w, G = g.new_face_vector(0), g.new_face_vector(0), g.new_face_vector(0), g.new_face_vector(0)
    U.set(0.5)
    nb = H.num_bfaces(0) * n ** (dim - 1)
    bd = g.new_boundary_vector(0, np.random.default_rng(1).uniform(-1, 1, nb))
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

    def recipe():
        g.gradient(p, G)
        G.multiply(w)
        U.addScaled(-0.25, G)

    def fused():
        g.project_weighted(U, p, w, alpha=0.25)

    wall = dict(recipe=[], fused=[])

    def rep(keep):
        g.apply(p, out)
        g.faces_from_cells(c, w, mode=capi.FACE_RECIP_MEAN)
        g.faces_from_cells(c, F, mode=capi.FACE_MEAN)
        g.gradient(p, G)
        g.project(U, p, alpha=0.25)
        g.add_boundary_rhs_weighted(bd, w, f)
        g.add_boundary_rhs(bd, f)
        g.sync()
        g.profile(False)  # (the recipe's launches stay out of the kernel rows: its gradient would be counted twice)
        t = timed(recipe)
        g.profile(True)
        t2 = timed(fused)
        if keep:
            wall["recipe"].append(t)
            wall["fused"].append(t2)

    g.profile(True)
    rep(False)
    g.sync()
    g.profile_reset()
    for _ in range(REPS):
        rep(True)
    rows = g.profile_rows()
    g.profile(False)

    def per_call(key):
        r = rows.get(key)
        return None if not r or not r["calls"] else r["ms"] / r["calls"]

    apply_ms = per_call("stencil_apply") or per_call("stencil_slabs")
    b = bytes_per_site(n, dim)
    result = dict(tool="tools/density_step_time.py", case=case, mesh=name, divides=div, n=n, dim=dim, sites=sites, reps=REPS, bytes_per_site=b,
                  apply_const_ms=round(apply_ms, 4), kernels={},
                  note="faces_from_cells: the mean of a MEAN and a RECIP_MEAN call per repetition; boundary_rhs_w / vecop(add_boundary_rhs): "
                       "boundary layers only, cells = boundary values")
    for key in ("faces_from_cells", "project_weighted", "gradient", "project"):
        ms = per_call(key)
        budget = 1.25 * (b[key] / b["apply"]) * apply_ms
        result["kernels"][key] = dict(ms=round(ms, 4), calls=rows[key]["calls"], budget_ms=round(budget, 4), fraction_of_budget=round(ms / budget, 3),
                                      tb_per_s=round(b[key] * sites / (ms * 1e-3) / 1e12, 3))
    # the fold touches the face layers of boundary patches only: 16 B per boundary cell (f read and written), 8 B datum, 8 B weight
    fold_bytes = 32.0 * nb / sites
    ms = per_call("boundary_rhs_w")
    budget = 1.25 * (fold_bytes / b["apply"]) * apply_ms
    result["kernels"]["boundary_rhs_w"] = dict(ms=round(ms, 4), calls=rows["boundary_rhs_w"]["calls"], bytes_per_site=round(fold_bytes, 4),
                                               budget_ms=round(budget, 4), fraction_of_budget=round(ms / budget, 3))
    result["projection"] = dict(fused_ms=round(float(np.median(wall["fused"])), 4), recipe_ms=round(float(np.median(wall["recipe"])), 4))
    result["projection"]["recipe_over_fused"] = round(result["projection"]["recipe_ms"] / result["projection"]["fused_ms"], 3)
    # what te_faces_from_cells replaces: a face vector built on the host and uploaded
    host = np.full(F.size, 1.25)
    ups = []
    for _ in range(5):
        g.sync()
        t0 = time.perf_counter()
        F.upload(host)
        g.sync()
        ups.append((time.perf_counter() - t0) * 1e3)
    result["upload_face_vector_ms"] = round(float(np.median(ups)), 3)
    result["face_vector_gib"] = round(F.size * 8 / 2 ** 30, 3)
    print(json.dumps(result), flush=True)
    return result


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "density_step_time.jsonl")
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
