"""CPU: (1) the numpy statement of gradient and divergence the GPU tests compare against (tests/projection_util.py) is pinned to the
reference's compiled operator: div(grad u) with the reference's own golden u and gamma gives its golden `apply` within the
operator-level tolerance, on every ref_*_n*.npz fixture, and the same with gamma from the oracle's interpolation; (2) the new entry
points exist, are bound, and refuse NULL arguments with TE_EINVAL without a device; (3) the C++ adaptor compiles against the
reference's headers."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from pressurepoissonsolver_amd import capi
from tests import projection_util as pu, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("THUNDEREGG_REF", "/root/reference")
FIXTURES = sorted(glob.glob(os.path.join(util.GOLDEN, "ref_*_n*.npz")))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def test_numpy_statement_reproduces_the_reference_apply(path):
    d = dict(np.load(path))
    dim, n = int(d["dim"]), int(d["n"])
    tol = 32 * util.EPS * 4 * dim / d["t_h"].min() ** 2 * np.abs(d["u"]).max()  # util.op_tol
    lo, hi = pu.grad(d["u"], d["t_h"], n, dim, d["t_nbr_kind"], d["t_neumann"], d["gamma"], d["iface_index"])
    err = np.abs(pu.div(lo, hi, d["t_h"], n, dim) - d["apply"]).max()
    Lg = orc.Level(dim, n, d["t_id"], d["t_h"], d["t_nbr_kind"], d["t_nbr"], d["t_nbr_orth"], d["t_neumann"], d["t_parent"], d["t_orth_on_parent"])
    assert util.op_tol(Lg, d["u"]) == tol
    u = util.rand_vec(Lg.size, 5)
    lo2, hi2 = pu.level_grad(Lg, u)
    err2 = np.abs(pu.level_div(Lg, lo2, hi2) - orc.apply(Lg, u)).max()
    tol2 = util.op_tol(Lg, u)
    print(f"{os.path.basename(path)}: golden u, gamma -> golden apply {err / tol:.3f} of op_tol; random u, oracle gamma -> oracle apply {err2 / tol2:.3f}")
    assert err <= tol and err2 <= tol2


def test_layout_helpers_round_trip():
    for n, dim, P in ((4, 3, 3), (6, 2, 5)):
        a = util.rand_vec(P * pu.face_size(n, dim), 1)
        lo, hi = pu.unpack(a, n, dim)
        assert np.array_equal(pu.pack(lo, hi), a)
        vlo, vhi = capi.face_vector_views(a, n, dim)
        assert capi.face_vector_size(n, dim) == pu.face_size(n, dim)
        assert np.array_equal(vlo, lo) and np.array_equal(vhi.reshape(hi.shape), hi)
        vlo[1, 0].flat[0] = 7.0  # views: a write lands in the host array, at LO_0 of patch 1
        assert a[pu.face_size(n, dim)] == 7.0


def test_entry_points_exist_and_refuse_null_arguments():
    L = capi.lib()
    for name in ("te_vec_create_faces", "te_gradient", "te_divergence", "te_project"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    out = C.c_void_p()
    assert L.te_vec_create_faces(None, 0, C.byref(out)) == capi.TE_EINVAL and not out.value
    assert L.te_gradient(None, 0, None, None, None) == capi.TE_EINVAL
    assert b"te_gradient" in L.te_last_error()
    assert L.te_divergence(None, 0, 1.0, None, None) == capi.TE_EINVAL
    assert b"te_divergence" in L.te_last_error()
    assert L.te_project(None, 0, 1.0, None, None, None) == capi.TE_EINVAL
    assert b"te_project" in L.te_last_error()
    for method in ("new_face_vector", "gradient", "divergence", "project"):
        assert callable(getattr(capi.GMG, method))
    hdr = open(os.path.join(ROOT, "include", "te_hip.h")).read()
    for decl in ("int    te_vec_create_faces(te_gmg *g, int level, te_vec **out);",
                 "int te_gradient(te_gmg *g, int level, const te_vec *u, const te_vec *bdata, te_vec *G);",
                 "int te_divergence(te_gmg *g, int level, double alpha, const te_vec *U, te_vec *out);",
                 "int te_project(te_gmg *g, int level, double alpha, const te_vec *p, const te_vec *bdata, te_vec *U);"):
        assert decl in hdr, decl


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src", "Thunderegg")), reason="reference tree not present")
def test_face_vector_adaptor_compiles_against_reference_headers():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-w", "-I" + os.path.join(REF, "src"), "-I/opt/conda/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pressurepoissonsolver_amd", "thunderegg"),
           os.path.join(ROOT, "tests", "projection_compile.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
