"""CPU: the float64 kernels of csrc/meshhole.hip compile without contracted multiply-adds, as tests/test_meshsubdiv_asm.py
checks for csrc/meshsubdiv.hip: the fused instructions the gfx950 assembly holds belong to the expansions of the square
roots (the edge lengths of `count`, the areas of `triangulate`), so their count per kernel equals that of a build with
contraction switched off for the whole translation unit.  The dynamic programme's W and split tables stay in LDS, under
the 40 KB a workgroup may take for several loops to share a CU."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "neuraludf_amd")
SRC = os.path.join(PKG, "csrc", "meshhole.hip")
KERNELS = {"hf_link_kernel", "hf_rank_kernel", "hf_count_kernel", "hf_triangulate_kernel"}


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def _per_kernel(tmp_path, extra):
    out = tmp_path / ("hf%d.s" % len(extra))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", str(out),
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(os.path.dirname(PKG), "include")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    counts, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = re.sub(r"^_Z\d+", "", m.group(1)).split("12NudfMeshTopo")[0]
            counts[cur] = dict(fused=0, mul=0)
        elif cur:
            counts[cur]["fused"] += bool(re.search(r"\bv_fmac?_f64\b", line))
            counts[cur]["mul"] += bool(re.search(r"\bv_mul_f64\b", line))
    return counts, text


def test_no_contracted_float64_multiply_add_and_lds_budget(tmp_path):
    built, text = _per_kernel(tmp_path, [])
    off, _ = _per_kernel(tmp_path, ["-ffp-contract=off"])
    assert KERNELS <= set(built), sorted(built)
    for k in KERNELS:
        assert built[k] == off[k], (k, built[k], off[k])
    assert built["hf_triangulate_kernel"]["mul"] > 0 and built["hf_count_kernel"]["mul"] > 0
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel _Z\d+(\w+?)12NudfMeshTopo.*?\.amdhsa_group_segment_fixed_size (\d+)", text, re.S)}
    assert 36 * 1024 <= lds["hf_triangulate_kernel"] < 40 * 1024, lds
    assert all(lds[k] == 0 for k in KERNELS - {"hf_triangulate_kernel"}), lds
