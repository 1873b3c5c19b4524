"""CPU: the float64 kernels of csrc/meshtexture.hip compile without contracted multiply-adds, as
tests/test_meshraster_asm.py checks for csrc/meshraster.hip: the fused instructions the gfx950 assembly holds belong to
the expansions of the division, the square root and pow, so their count per kernel equals that of a build with
contraction switched off for the whole translation unit."""
import os
import re
import subprocess

from test_meshraster_asm import PKG, _hipcc

SRC = os.path.join(PKG, "csrc", "meshtexture.hip")
KERNELS = {"tx_bake_kernel", "tx_shade_kernel"}


def _per_kernel(tmp_path, extra):
    out = tmp_path / ("tx%d.s" % len(extra))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", str(out),
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(os.path.dirname(PKG), "include")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = re.sub(r"^_Z\d+", "", m.group(1)).split("14NudfMeshRaster")[0]
            counts[cur] = dict(fused=0, mul=0)
        elif cur:
            counts[cur]["fused"] += bool(re.search(r"\bv_fmac?_f64\b", line))
            counts[cur]["mul"] += bool(re.search(r"\bv_mul_f64\b", line))
    return counts


def test_no_contracted_float64_multiply_add(tmp_path):
    built = _per_kernel(tmp_path, [])
    off = _per_kernel(tmp_path, ["-ffp-contract=off"])
    assert KERNELS <= set(built), sorted(built)
    for k in KERNELS:
        assert built[k] == off[k], (k, built[k], off[k])
    assert built["tx_bake_kernel"]["mul"] >= 6 + 9 + 9 + 4 + 12            # edge functions, point, projection, weights, mix
    assert built["tx_shade_kernel"]["mul"] >= 6 + 4 + 12                   # UV, weights, mix
