"""CPU: the float64 kernels of csrc/meshwinding.hip compile without contracted multiply-adds, as
tests/test_meshintersect_asm.py checks for csrc/meshintersect.hip: the fused instructions the gfx950 assembly holds belong
to the expansions of the correctly rounded divisions and square roots and to atan2, so their count per kernel equals that
of a build with contraction switched off for the whole translation unit.  A decision of the walk must not depend on
whether a product was rounded.  The kernels use no scratch memory: the moments and the node record live in registers."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "neuraludf_amd")
SRC = os.path.join(PKG, "csrc", "meshwinding.hip")
KERNELS = {"pc_wn_faces_kernel", "pc_wn_nodes_kernel", "pc_winding_kernel"}


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def _per_kernel(tmp_path, extra):
    out = tmp_path / ("mw%d.s" % len(extra))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", str(out),
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(os.path.dirname(PKG), "include")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    counts, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = re.sub(r"^_Z\d+", "", m.group(1)).split("14NudfPointCloud")[0]
            counts[cur] = 0
        elif cur:
            counts[cur] += bool(re.search(r"\bv_fmac?_f64\b", line))
    return counts, text


def test_no_contracted_float64_multiply_add_and_no_scratch(tmp_path):
    built, text = _per_kernel(tmp_path, [])
    off, _ = _per_kernel(tmp_path, ["-ffp-contract=off"])
    assert KERNELS <= set(built), sorted(built)
    for k in KERNELS:
        assert built[k] == off[k], (k, built[k], off[k])
    size = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel _Z\d+(\w+?)14NudfPointCloud.*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S)}
    assert set(size) == KERNELS and all(v == 0 for v in size.values()), size
    meta = [int(x) for x in re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M)]
    assert len(meta) == len(KERNELS) and all(v == 0 for v in meta), meta
