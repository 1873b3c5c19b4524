"""CPU: the float64 kernels of csrc/meshdist.hip compile without contracted multiply-adds (what
tests/test_pointcloud_asm.py checks for csrc/pointcloud.hip).  The fused instructions the gfx950 assembly does hold
belong to the correctly rounded division and square-root expansions: their count per kernel equals that of a build with
contraction switched off for the whole translation unit."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "neuraludf_amd")
SRC = os.path.join(PKG, "csrc", "meshdist.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def _fused_per_kernel(tmp_path, extra):
    out = tmp_path / ("md%d.s" % len(extra))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", str(out),
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(os.path.dirname(PKG), "include")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = re.sub(r"^_Z\d+", "", m.group(1)).split("14NudfPointCloud")[0]
            counts[cur] = dict(fused=0, div=0, sqrt=0)
        elif cur:
            counts[cur]["fused"] += bool(re.search(r"\bv_fmac?_f64\b", line))
            counts[cur]["div"] += "v_div_fixup_f64" in line
            counts[cur]["sqrt"] += "v_rsq_f64" in line
    return counts


def test_no_contracted_float64_multiply_add(tmp_path):
    built = _fused_per_kernel(tmp_path, [])
    off = _fused_per_kernel(tmp_path, ["-ffp-contract=off"])
    kernels = {"pc_tribin_count_kernel", "pc_tribin_emit_kernel", "pc_closest_kernel"}
    assert kernels <= set(built), sorted(built)
    for k in kernels:
        assert built[k] == off[k], (k, built[k], off[k])
        if built[k]["div"] == 0 and built[k]["sqrt"] == 0:
            assert built[k]["fused"] == 0, (k, built[k])
    assert built["pc_closest_kernel"]["div"] > 0 and built["pc_closest_kernel"]["sqrt"] > 0
