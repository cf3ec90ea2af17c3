"""Tooling: the cycle and the BiCGStab + GMG solve under the channel mask (Neumann on every side but the top) next to the
all-Dirichlet domain, same process, same box, both smoothers; plus one fold of boundary data (te_add_boundary_rhs). 512^3 in 32^3
patches by default. One JSON line per (mask, smoother). For the record, not a target: under the reference smoother the patches along
Neumann sides take k_ps_fused instead of k_ps_sym, as on an all-Neumann domain. argv: [divides] (default 4: 512^3; 3: 256^3)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
from pressurepoissonsolver_amd import capi  # noqa: E402


def timed(g, fn, reps):
    fn()
    g.sync()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    g.sync()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    div = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    mesh = capi.Mesh.uniform(3, div)
    for name, mask in (("dirichlet", 0), ("channel", 0b011111)):
        H = capi.Hierarchy(mesh, 32, neumann_sides=mask)
        g = capi.GMG(H)
        f, u, bd = g.new_vector(0), g.new_vector(0), g.new_boundary_vector(0)
        g.init_problem_sides(f)
        g.boundary_sample(bd)
        fold_ms = timed(g, lambda: g.add_boundary_rhs(bd, u), 20)
        for sm_name, sm in (("patch_solve", capi.SMOOTH_PATCH_SOLVE), ("rbgs", capi.SMOOTH_RBGS)):
            o = g.default_opts(smoother=sm)
            cycle_ms = timed(g, lambda: g.cycle(o, f, u), 20)
            g.bicgstab(u, f, o, tol=1e-12)
            u.set(0.0)
            g.sync()
            t = time.perf_counter()
            its, rr = g.bicgstab(u, f, o, tol=1e-12)
            g.sync()
            print(json.dumps(dict(cells=H.cells(0), mask=name, smoother=sm_name, cycle_ms=round(cycle_ms, 4), solve_ms=round((time.perf_counter() - t) * 1e3, 3),
                                  its=its, rel=rr, fold_ms=round(fold_ms, 4), bfaces=H.num_bfaces(0))), flush=True)
        del f, u, bd, g


if __name__ == "__main__":
    main()
