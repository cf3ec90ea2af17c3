"""CPU: the C-ABI library loads, exports every symbol include/te_hip.h declares, and refuses to
run without a GPU (no CPU fallback). No compute entry point is called here."""
import ctypes as C
import os
import re

import pytest

from pressurepoissonsolver_amd import capi
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "te_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(te_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    decl = declared_symbols()
    assert len(decl) >= 50
    assert sorted(capi.SYMBOLS) == decl


def test_every_symbol_exported():
    lib = C.CDLL(capi.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), name


def test_error_convention_and_no_cpu_fallback():
    with pytest.raises(capi.TeError) as e:
        capi.Mesh.read("/nonexistent/mesh.bin", 3)
    assert e.value.code == capi.TE_EIO
    with pytest.raises(capi.TeError) as e:
        capi.Hierarchy(util.mesh("2uni.bin"), 7)  # odd n
    assert e.value.code == capi.TE_EINVAL
    import torch
    if not torch.cuda.is_available():
        H = capi.Hierarchy(util.mesh("2uni.bin"), 8)
        with pytest.raises(capi.TeError) as e:
            capi.GMG(H)
        assert e.value.code == capi.TE_EHIP  # fails loudly: no device, no fallback


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pressurepoissonsolver_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "te_oracle" not in text and "from oracle" not in text and "import oracle" not in text, f


def test_no_getenv_on_launch_paths():
    """the TE_* switches are read once (te_gmg_create -> Cfg::fromEnv; te_hier_build for the partition), never per launch"""
    src = _device_sources()
    calls = [ln for ln in src.splitlines() if "getenv(" in ln]
    assert len(calls) == 1 and "optName[o]" in calls[0], calls
    for hdr in os.listdir(os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")):
        if hdr.endswith(".hpp"):
            assert "getenv(" not in open(os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc", hdr)).read(), hdr


def _device_sources():
    """the translation units of the device half of the library (pressurepoissonsolver_amd/build.py UNITS), concatenated"""
    d = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")
    return "\n".join(open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.startswith("gmg_") and f.endswith(".hip"))


def test_every_extern_c_entry_has_an_exception_barrier():
    """no C++ exception may unwind into a C caller: every int-returning entry point of the device units runs inside guarded()"""
    body = _device_sources()
    entries = re.findall(r"^int\s+(te_\w+)\(", body, flags=re.M)
    assert len(entries) >= 40
    for name in entries:
        at = re.search(r"^int\s+" + name + r"\([^{;]*\)\s*\{(.{0,80})", body, flags=re.M | re.S)
        assert at and "guarded(" in at.group(1), name


@pytest.mark.gpu
def test_set_option_and_release_workspace():
    H = capi.Hierarchy(util.mesh("2uni.bin"), 8)
    g = capi.GMG(H)
    g.set_option("TE_NO_FCORR", "1")
    g.set_option("TE_NO_FCORR", None)
    with pytest.raises(capi.TeError) as e:
        g.set_option("TE_NO_SUCH_SWITCH", "1")
    assert e.value.code == capi.TE_EINVAL
    with pytest.raises(capi.TeError) as e:
        g.set_option("TE_2D_SIMPLE", "1")  # shapes the level tables: fixed at creation
    assert e.value.code == capi.TE_ESTATE
    # te_gmg_slab_count: what the slab rules give a level as the switches stand (a handful of 8^3 patches: two slabs)
    assert g.slab_count(0, capi.SLABS_STENCIL) == 2 and g.slab_count(0, capi.SLABS_SWEEP) == 2
    g.set_option("TE_ZS_PIN", "1")
    assert g.slab_count(0, capi.SLABS_STENCIL) == 1 and g.slab_count(0, capi.SLABS_SWEEP) == 1
    g.set_option("TE_ZS_PIN", None)
    with pytest.raises(capi.TeError) as e:
        g.set_option("TE_ZS_PIN", "3")
    assert e.value.code == capi.TE_EINVAL and g.slab_count(0) == 2
    # TE_RESWEEP_V: 19, 27 or 59, the post-sweep variants a default reaches; a retired switch is an unknown option
    with pytest.raises(capi.TeError) as e:
        g.set_option("TE_RESWEEP_V", "31")
    assert e.value.code == capi.TE_EINVAL
    g.set_option("TE_RESWEEP_V", "59")
    g.set_option("TE_RESWEEP_V", None)
    with pytest.raises(capi.TeError) as e:
        g.set_option("TE_NO_GTAB2", "1")
    assert e.value.code == capi.TE_EINVAL
    from pressurepoissonsolver_amd import problems
    f, _ = problems.init_dirichlet(H.tables(0), 8)
    x = g.new_vector(0)
    its, rr = g.bicgstab(x, g.new_vector(0, f), g.default_opts())
    g.release_workspace()
    x2 = g.new_vector(0)
    its2, rr2 = g.bicgstab(x2, g.new_vector(0, f), g.default_opts())  # allocates them again
    assert its2 == its and (x2.download() == x.download()).all()


def test_header_is_valid_c99():
    """include/te_hip.h is a C header: plain pointers, sizes and opaque handles (what a cgo / JNI / ctypes binding consumes)"""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "hdr.c")
        open(src, "w").write('#include "te_hip.h"\nint main(void) { te_cycle_opts o; te_cycle_opts_default(&o); return TE_OK; }\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_host_mesh_code_is_clean_under_sanitizers():
    """the host-only half of the library (csrc/mesh.cpp, capi_mesh.cpp) built with -fsanitize=address,undefined and driven
    through the C ABI over every mesh fixture, deep AMR trees and --divide included, 1 / 2 / 3 / 8 ranks (tests/host_sanitize.cpp)"""
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "host_sanitize")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_sanitize.cpp"),
                            os.path.join(csrc, "capi_mesh.cpp"), os.path.join(csrc, "mesh.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        args = []
        for name, dim, div in (("2refine.bin", 3, 2), ("multi_refine.bin", 3, 1), ("multi_refine_8.bin", 3, 0),
                               ("2d_multi_refine_8.bin", 2, 1), ("2d2ref.bin", 2, 3), ("3uni.bin", 3, 1), ("1uni.bin", 3, 3)):
            args += [os.path.join(util.GOLDEN, name), str(dim), str(div)]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0 and "SANITIZE_OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


@pytest.mark.gpu
def test_setup_breakdown_and_event_stride():
    """te_gmg_setup_ms: the parts of te_gmg_create add up to its total, and a second solver in the same process costs a small
    fraction of the first (whose context part carries the HIP runtime's start and the code-object load);
    te_gmg_profile_stride: only every n-th launch of a class is timed and counted, the averages stay what they are"""
    H = capi.Hierarchy(util.mesh("uniform", 3), 8)
    g1 = capi.GMG(H)
    g2 = capi.GMG(H)
    for g in (g1, g2):
        p = g.setup_ms()
        assert p["device_allocation_count"] > 20 and p["total"] > 0
        parts = sum(p[k] for k in ("context_streams", "host_tables", "device_allocations", "table_uploads", "work_vectors", "final_sync"))
        assert abs(parts - p["total"]) <= 0.05 * p["total"] + 0.05
    assert g2.setup_ms()["total"] < 100.0  # (milliseconds: nothing of a process's first HIP call is in a second create)
    f, u = g2.new_vector(0, util.rand_vec(H.cells(0), 3)), g2.new_vector(0)
    o = g2.default_opts(smoother=capi.SMOOTH_RBGS)
    rows = {}
    for stride in (1, 4):
        g2.profile(True)
        g2.profile_stride(stride)
        g2.profile_reset()
        for _ in range(8):
            g2.cycle(o, f, u)
        rows[stride] = g2.profile_rows()
        g2.profile(False)
    g2.profile_stride(1)
    for k, v in rows[1].items():
        assert v["calls"] % 8 == 0
        assert rows[4][k]["calls"] == v["calls"] // 4, (k, v["calls"], rows[4][k]["calls"])
        assert rows[4][k]["cells"] * v["calls"] == v["cells"] * rows[4][k]["calls"] or len({rows[4][k]["cells"] // rows[4][k]["calls"], v["cells"] // v["calls"]}) <= 2
