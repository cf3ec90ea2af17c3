"""Tooling: te_gradient, te_divergence and te_project next to te_apply (existing code: the yardstick with the same read side) and next
to what a driver pays today per field, a te_vec_download + te_vec_upload of one domain vector. HIP-event times from the library's
own profile rows, the four operations alternating in one process, REPS repetitions after a warm-up. Cases: 512^3 in 32^3 patches,
2refine.bin --divide 3 in 32^3 patches, 2D 4096^2 in 64^2 patches. One JSON line per case, appended to
profiles/projection_bench.jsonl. Acceptance of each new kernel: time <= 1.25 x (its algorithmic bytes / te_apply's) x te_apply's
time from the same run (`ratio_to_budget` <= 1). argv: [case ...] (default: all of 512 2refine 2d)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 20, 3


def algorithmic_bytes(n, dim):
    """per lattice site: one value per cell, 2 dim halo layers read, dim HI layers of a face vector"""
    halo, hi = 2 * dim / n * 8, dim / n * 8
    face = dim * 8 + hi
    return dict(stencil_apply=8 + halo + 8, gradient=8 + halo + face, divergence=face + 8, project=8 + halo + 2 * face)


def mesh_of(case):
    if case == "512":
        return capi.Mesh.uniform(3, 4), 32
    if case == "2refine":
        m = capi.Mesh.read(os.path.join(ROOT, "tests", "golden", "2refine.bin"), 3)
        for _ in range(3):
            m.refine_leaves()
        return m, 32
    if case == "2d":
        return capi.Mesh.uniform(2, 6), 64
    raise SystemExit(f"unknown case {case}")


def run(case):
    m, n = mesh_of(case)
    H = capi.Hierarchy(m, n)
    g = capi.GMG(H)
    u, out, G = g.new_vector(0), g.new_vector(0), g.new_face_vector(0)
    g.init_problem(u, problem=capi.PROBLEM_RANDOM)
    ops = dict(stencil_apply=lambda: g.apply(u, out), gradient=lambda: g.gradient(u, G), divergence=lambda: g.divergence(G, out),
               project=lambda: g.project(G, u, alpha=1e-3))
    for _ in range(WARM):
        for f in ops.values():
            f()
    g.sync()
    g.profile(True)
    g.profile_reset()
    for _ in range(REPS):
        for f in ops.values():
            f()
    rows = g.profile_rows()
    g.profile(False)
    host = np.empty(u.size)
    t = time.perf_counter()
    for _ in range(3):
        capi.check(capi.lib().te_vec_download(u.h, host.ctypes.data_as(capi.C.c_void_p)))
        capi.check(capi.lib().te_vec_upload(u.h, host.ctypes.data_as(capi.C.c_void_p)))
    round_trip_ms = (time.perf_counter() - t) * 1e3 / 3
    by = algorithmic_bytes(n, H.dim)
    ms = {k: rows[k]["ms"] / rows[k]["calls"] for k in ops}
    res = dict(case=case, dim=H.dim, n=n, cells=H.cells(0), reps=REPS, ms={k: round(v, 4) for k, v in ms.items()},
               bytes_per_site={k: round(v, 3) for k, v in by.items()},
               tb_per_s={k: round(by[k] * H.cells(0) / (ms[k] * 1e-3) / 1e12, 3) for k in ops},
               ratio_to_budget={k: round(ms[k] / (1.25 * by[k] / by["stencil_apply"] * ms["stencil_apply"]), 3) for k in ops if k != "stencil_apply"},
               download_upload_ms=round(round_trip_ms, 3))
    res["accepted"] = all(v <= 1.0 for v in res["ratio_to_budget"].values())
    return res


def main():
    cases = sys.argv[1:] or ["512", "2refine", "2d"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for case in cases:
        line = json.dumps(run(case))
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "projection_bench.jsonl"), "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
