"""Tooling: what a regrid costs on the device. Uniform meshes in 32^3 patches, destination of size^3 cells unless said otherwise, the
three kinds of te_vec_regrid each on its own -- copy (size^3 -> the same mesh on a second solver), refine ((size/2)^3 -> size^3, every
leaf refined), coarsen (size^3 -> (size/2)^3, every family coarsened) -- beside a flat te_vec_copy of a size^3 vector and
te_patch_indicator on size^3, and the same three kinds of te_faces_regrid on face vectors (filled by te_gradient of the random vector),
alternating in one process, REPS repetitions after a warm-up round. Kernel times from the library's
profile rows (HIP events around each launch); the indicator's wall time includes its synchronisation and the copy of one double per
patch to the host. Writes profiles/regrid.json.

    python tools/regrid_time.py [--out PATH] [sizes ...]        (default: 256 512)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pressurepoissonsolver_amd import capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
N = 32
# algorithmic bytes per DESTINATION site: copy reads and writes a value; refine writes one, reads 1/8 of a source value plus the ring
# of the octant ((18^3 - 16^3) / 32^3 values); coarsen writes one and reads eight
BYTES = dict(copy=16.0, refine=8 + 8 * 18 ** 3 / N ** 3, coarsen=72.0, flat_copy=16.0, indicator=8.0)
# te_faces_regrid, per destination site = a cell with its three lower faces and its share of the HI blocks (24 + 24/32 B): copy reads and
# writes that; refine writes it and reads, per component, the octant's block of 17 x 18 x 18 values; coarsen reads four fine faces per face
FACE = 24.0 + 24.0 / N
BYTES.update(faces_copy=2 * FACE, faces_refine=FACE + 3 * 8 * 17 * 18 * 18 / N ** 3, faces_coarsen=5 * FACE)


def solver(divides):
    m = capi.Mesh.uniform(3, divides)
    H = capi.Hierarchy(m, N)
    return m, H, capi.GMG(H)


def run(size):
    d = int(round(np.log2(size // N)))
    m, H, g = solver(d)
    _, H_same, g_same = solver(d)
    m_half, H_half, g_half = solver(d - 1)
    u, v, u_same, u_half = g.new_vector(0), g.new_vector(0), g_same.new_vector(0), g_half.new_vector(0)
    g.init_problem(u, None, problem=capi.PROBLEM_RANDOM)
    g_half.init_problem(u_half, None, problem=capi.PROBLEM_RANDOM)
    # the meshes are one adapt apart: the tool's own check that it times what it says
    assert list(m_half.adapt({int(i): 1 for i in m_half.leaves()}).leaves()) == list(m.leaves())
    ops = dict(copy=(g_same, lambda: capi.regrid(g, u, g_same, u_same), "regrid", H.cells(0)),
               refine=(g, lambda: capi.regrid(g_half, u_half, g, v), "regrid", H.cells(0)),
               coarsen=(g_half, lambda: capi.regrid(g, u, g_half, u_half), "regrid", H_half.cells(0)),
               flat_copy=(g, lambda: v.copy(u), "vecop", H.cells(0)),
               indicator=(g, lambda: g.patch_indicator(u), "indicator", H.cells(0)))
    # and that the instantiations it times (one slab per patch at these sizes) compute what they should: a copy has the source's
    # checksum, a coarsening te_restrict's on the source solver, and refining then coarsening gives back the cell means' parents
    capi.regrid(g, u, g_same, u_same)
    assert u_same.checksumLocal() == u.checksumLocal(), "copy differs from its source"
    r, keep = g.new_vector(1), g_half.new_vector(0)
    g.restrict(r, u, fine_level=0)
    keep.copy(u_half)
    capi.regrid(g, u, g_half, u_half)
    assert u_half.checksumLocal() == r.checksumLocal(), "coarsen differs from te_restrict"
    u_half.copy(keep)
    capi.regrid(g_half, u_half, g, v)
    # (per axis the weights' absolute sum is at most (30 + 5 * 7 + 3) / 32: an extrapolated ghost, weight 3 + 3 + 1, under the 5/32 tap)
    assert np.isfinite(v.infNorm()) and v.infNorm() <= 2.125 ** 3 * u_half.infNorm(), "refine is out of its bound"
    del r, keep
    # face vectors: the gradients of the random vectors; a copy has the source's checksum, and refining keeps the divergence of
    # every cell (so its maximum) to rounding
    U, V, U_same, U_half = g.new_face_vector(0), g.new_face_vector(0), g_same.new_face_vector(0), g_half.new_face_vector(0)
    g.gradient(u, U)
    g_half.gradient(u_half, U_half)
    capi.regrid_faces(g, U, g_same, U_same)
    assert U_same.checksumLocal() == U.checksumLocal(), "face copy differs from its source"
    capi.regrid_faces(g_half, U_half, g, V)
    d, d_half = g.new_vector(0), g_half.new_vector(0)
    g.divergence(V, d)
    g_half.divergence(U_half, d_half)
    assert abs(d.infNorm() - d_half.infNorm()) <= 1e-9 * d_half.infNorm(), "face refinement changed the divergence"
    del d, d_half
    ops.update(faces_copy=(g_same, lambda: capi.regrid_faces(g, U, g_same, U_same), "regrid_faces", H.cells(0)),
               faces_refine=(g, lambda: capi.regrid_faces(g_half, U_half, g, V), "regrid_faces", H.cells(0)),
               faces_coarsen=(g_half, lambda: capi.regrid_faces(g, U, g_half, U_half), "regrid_faces", H_half.cells(0)))
    out = dict(size=size, n=N, patches=H.sizes(0)[1], reps=REPS, kinds={})
    for name, (gg, fn, row, sites) in ops.items():
        for _ in range(3):
            fn()
        gg.sync()
        gg.profile(True)
        gg.profile_select(row)
        gg.profile_reset()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        gg.sync()
        wall = (time.perf_counter() - t0) / REPS * 1e3
        r = gg.profile_rows()[row]
        gg.profile(False)
        gg.profile_select(None)
        ms = r["ms"] / r["calls"]
        out["kinds"][name] = dict(kernel_ms=round(ms, 4), wall_ms_per_call=round(wall, 4), destination_sites=sites, bytes_per_site=round(BYTES[name], 3),
                                  tb_per_s=round(BYTES[name] * sites / (ms * 1e-3) / 1e12, 3))
    flat = out["kinds"]["flat_copy"]["kernel_ms"]
    for name in ("copy", "refine", "coarsen", "faces_copy", "faces_refine", "faces_coarsen"):
        k = out["kinds"][name]
        k["ratio_to_flat_copy_per_byte"] = round((k["kernel_ms"] / (k["bytes_per_site"] * k["destination_sites"])) / (flat / (16.0 * H.cells(0))), 3)
    print(f"{size}^3: " + "; ".join(f"{k}: {v['kernel_ms']:.3f} ms ({v['tb_per_s']:.2f} TB/s)" for k, v in out["kinds"].items()), flush=True)
    return out


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "regrid.json")
    if args and args[0] == "--out":
        path, args = os.path.abspath(args[1]), args[2:]
    sizes = [int(a) for a in args] or [256, 512]
    result = dict(tool="tools/regrid_time.py", setup="uniform meshes, 32^3 patches; te_vec_regrid and te_faces_regrid per kind, te_vec_copy, te_patch_indicator", runs=[run(s) for s in sizes])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
