"""CPU: the float64 kernels of csrc/meshorient.hip -- the outward sum and the vertex normals -- compile without contracted
multiply-adds, as tests/test_meshclean_asm.py checks for csrc/meshtopo.hip: the fused instructions the gfx950 assembly
holds belong to the expansions of the division, the square root and atan2, so their count per kernel equals that of a
build with contraction switched off for the whole translation unit, and the integer kernels hold none."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "neuraludf_amd")
SRC = os.path.join(PKG, "csrc", "meshorient.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def _per_kernel(tmp_path, extra):
    out = tmp_path / ("mo%d.s" % len(extra))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", str(out),
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(os.path.dirname(PKG), "include")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = re.sub(r"^_Z\d+", "", m.group(1)).split("14NudfMeshOrient")[0]
            counts[cur] = dict(fused=0, mul=0)
        elif cur:
            counts[cur]["fused"] += bool(re.search(r"\bv_fmac?_f64\b", line))
            counts[cur]["mul"] += bool(re.search(r"\bv_mul_f64\b", line))
    return counts


def test_no_contracted_float64_multiply_add(tmp_path):
    built = _per_kernel(tmp_path, [])
    off = _per_kernel(tmp_path, ["-ffp-contract=off"])
    kernels = {"mo_hook_kernel", "mo_jump_kernel", "mo_check_kernel", "mo_outward_kernel", "mo_normals_kernel"}
    assert kernels <= set(built), sorted(built)
    for k in kernels:
        assert built[k] == off[k], (k, built[k], off[k])
    for k in ("mo_hook_kernel", "mo_jump_kernel", "mo_check_kernel"):
        assert built[k] == dict(fused=0, mul=0), (k, built[k])
    assert built["mo_outward_kernel"]["mul"] >= 9            # six products of the cross product, three of the dot product
    assert built["mo_normals_kernel"]["mul"] >= 18
