"""CPU (hipcc cross-compiles gfx950): the generated code of the linear-prolongation kernels (csrc/prolongkernels.hpp). (1) No
instantiation uses scratch memory or spills a register, and the staged ring block fits the 64 KiB of static LDS. (2) The march of
k_prolong_linear3d keeps its fine planes in flight: a step consumes the four pairs requested two steps earlier, and behind them
the step before has issued its four loads and four stores -- at every wait inside the march those eight may still be in
flight (the floor follows from the request pattern, not from a measurement)                                          -> vmcnt >= 8
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pressurepoissonsolver_amd", "csrc", "gmg_prolong.hip")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("isa") / "prolong.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().split("\n")


def test_no_scratch_no_spills_and_lds_fits(asm):
    meta, cur, lds = {}, {}, 0
    for l in asm:  # the kernels' metadata records, fields in alphabetical order: the LDS size, then .name, then the other sizes
        m = re.match(r"^\s+\.(name|group_segment_fixed_size|private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", l)
        if not m:
            continue
        if m.group(1) == "group_segment_fixed_size":
            lds = int(m.group(2))
        elif m.group(1) == "name":
            cur = meta.setdefault(m.group(2), dict(lds=lds))
        else:
            cur[m.group(1)] = int(m.group(2))
    ours = {k: v for k, v in meta.items() if "k_prolong_linear" in k}
    assert len(ours) == 11, sorted(ours)  # 3D: n = 4 (1 slab count), 8 (2), 16 (3), 32 (4); 2D: one kernel
    for name, v in ours.items():
        assert (v["private_segment_fixed_size"], v["sgpr_spill_count"], v["vgpr_spill_count"]) == (0, 0, 0), (name, v)
        assert v["lds"] <= 64 * 1024, (name, v)
    lds32 = next(v["lds"] for k, v in ours.items() if "k_prolong_linear3dILi32ELi1E" in k)
    assert lds32 == 18 ** 3 * 8  # the ring block of an octant of a 32^3 patch


def loops(body):
    """(first line, last line) of every loop: the backward branches into blocks the compiler's comments assign to one header"""
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l)
        if m:
            h = re.search(r"Header=BB(\d+_\d+)", m.group(2))
            labels[m.group(1)] = (i, ".LBB" + h.group(1) if h else (m.group(1) if "Loop Header" in m.group(2) else None))
    out = {}
    for i, l in enumerate(body):
        m = re.search(r"(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(2) in labels and labels[m.group(2)][0] < i and labels[m.group(2)][1]:
            t, header = labels[m.group(2)]
            s0, e0 = out.get(header, (t, i))
            out[header] = (min(s0, t), max(e0, i))
    return list(out.values())


@pytest.mark.parametrize("frag", ["k_prolong_linear3dILi32ELi1E", "k_prolong_linear3dILi32ELi2E", "k_prolong_linear3dILi16ELi1E"])
def test_march_never_waits_for_the_loads_of_its_own_step(asm, frag):
    starts = [(i, l.split(":")[0]) for i, l in enumerate(asm) if re.match(r"^_ZN2te\w+:", l)]
    k = next((k for k, (i, n) in enumerate(starts) if frag in n), None)
    assert k is not None, f"{frag} is not instantiated"
    i = starts[k][0]
    j = starts[k + 1][0] if k + 1 < len(starts) else len(asm)
    body = asm[i:next((e for e in range(i, j) if asm[e].startswith(".Lfunc_end")), j)]
    # the march: the loop that reads the LDS block and stores to global memory (two steps per iteration: 8 pair loads, 8 pair stores)
    march = [(s, e) for s, e in loops(body) if any("ds_read" in l for l in body[s:e + 1]) and any("global_store" in l for l in body[s:e + 1])]
    assert len(march) == 1, march
    seg = body[march[0][0]:march[0][1] + 1]
    assert sum("global_load_dwordx4" in l for l in seg) == 8 and sum("global_store_dwordx4" in l for l in seg) == 8
    w = [int(m.group(1)) for l in seg for m in [re.search(r"s_waitcnt\s+vmcnt\((\d+)\)", l)] if m]
    assert w and min(w) >= 8, sorted(set(w))
