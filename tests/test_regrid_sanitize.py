"""CPU: te_mesh_adapt, te_mesh_leaves, te_mesh_is_balanced, te_hier_leaf_tree and te_hier_build on adapted trees are clean under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/host_sanitize_adapt.cpp, a stand-alone program over csrc/mesh.cpp and
csrc/capi_mesh.cpp built with g++, run over every mesh fixture. Nothing is loaded into python."""
import glob
import os
import subprocess

from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapt_is_clean_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc")
    exe = str(tmp_path / "host_sanitize_adapt")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_sanitize_adapt.cpp"),
                        os.path.join(csrc, "capi_mesh.cpp"), os.path.join(csrc, "mesh.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args = []
    for f in sorted(glob.glob(os.path.join(util.GOLDEN, "*.bin"))):
        args += [f, "2" if os.path.basename(f).startswith("2d") else "3"]
    assert len(args) >= 18
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0 and "SANITIZE_OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
