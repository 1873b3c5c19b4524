"""CPU: the float64 kernels of csrc/meshintersect.hip compile without contracted multiply-adds, as tests/test_meshhole_asm.py
checks for csrc/meshhole.hip: the fused instructions the gfx950 assembly holds belong to the expansions of the correctly
rounded divisions (the cell coordinates of the broad phase), so their count per kernel equals that of a build with
contraction switched off for the whole translation unit.  A sign must not depend on whether a product was rounded.  The
corners of a triangle are picked value by value, never through a pointer into a private array: the kernels use no scratch
memory and no LDS."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "neuraludf_amd")
SRC = os.path.join(PKG, "csrc", "meshintersect.hip")
KERNELS = {"pc_isect_count_kernel", "pc_isect_emit_kernel"}


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def _per_kernel(tmp_path, extra):
    out = tmp_path / ("mi%d.s" % len(extra))
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
            counts[cur] = dict(fused=0, mul=0)
        elif cur:
            counts[cur]["fused"] += bool(re.search(r"\bv_fmac?_f64\b", line))
            counts[cur]["mul"] += bool(re.search(r"\bv_mul_f64\b", line))
    return counts, text


def test_no_contracted_float64_multiply_add_no_scratch_no_lds(tmp_path):
    built, text = _per_kernel(tmp_path, [])
    off, _ = _per_kernel(tmp_path, ["-ffp-contract=off"])
    assert KERNELS <= set(built), sorted(built)
    for k in KERNELS:
        assert built[k] == off[k], (k, built[k], off[k])
        assert built[k]["mul"] > 100, (k, built[k])              # the predicates are there, inlined
    for field in ("private_segment_fixed_size", "group_segment_fixed_size"):
        size = {m.group(1): int(m.group(2)) for m in re.finditer(
            r"\.amdhsa_kernel _Z\d+(\w+?)14NudfPointCloud.*?\.amdhsa_%s (\d+)" % field, text, re.S)}
        assert set(size) == KERNELS and all(v == 0 for v in size.values()), (field, size)
    assert not re.search(r"\bscratch_(load|store)", text)
    for k in KERNELS:                                             # no stack that the size above would not show
        assert re.search(r"\.amdhsa_kernel _Z\d+%s14NudfPointCloud.*?\.amdhsa_uses_dynamic_stack 0" % k, text, re.S), k
