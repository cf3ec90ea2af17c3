"""CPU: csrc/dispatch.hpp, the one place that maps a run-time patch size and z-slab count to a kernel instantiation, checked by
tests/dispatch_host.cpp -- a stand-alone program built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer (the header
is plain C++17 and needs no HIP). A static_assert in the program's functor proves that no forbidden (N, ZS) pair is ever
instantiated, so building it is part of the test. Nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_helpers(tmp_path):
    exe = str(tmp_path / "dispatch_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc"), os.path.join(ROOT, "tests", "dispatch_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "DISPATCH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
