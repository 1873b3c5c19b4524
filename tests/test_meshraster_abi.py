"""CPU: the ctypes mirror of NudfMeshRaster (neuraludf_amd/_lib.py) against a C compile of include/nudf.h -- field names,
offsets and size --, the exports, the struct size the loader checks, the launchers' host-side size checks, and the
library version, which this block leaves alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("project", "bounds", "draw_small", "draw_large", "resolve", "visible", "colour")


def test_meshraster_struct_matches_the_header(tmp_path):
    from neuraludf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nudf.h")).read()
    body = re.search(r"typedef struct NudfMeshRaster \{(.*?)\} NudfMeshRaster;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", d)[-1] for d in body.split(";") if d.strip()]       # `fill[3]` -> fill
    assert names == [f[0] for f in _lib.MeshRaster._fields_]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this box")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nudf.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(NudfMeshRaster));']
    lines += ['  printf("%s %%zu\\n", offsetof(NudfMeshRaster, %s));' % (n, n) for n in names]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.MeshRaster)
    for n in names:
        assert int(got[n]) == getattr(_lib.MeshRaster, n).offset, n


def test_exports_struct_size_and_version():
    from neuraludf_amd import build, _lib
    build.build()
    lib = _lib.lib()
    assert lib.nudf_version() == _lib.ABI_VERSION == 108
    for s in ["nudf_meshraster_struct_size"] + ["nudf_meshraster_" + e for e in ENTRIES]:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.nudf_meshraster_struct_size() == C.sizeof(_lib.MeshRaster)
    assert "meshraster.hip" in build.SOURCES
    assert {"csrc/meshraster.hip", "csrc/meshraster_pixel.h"} <= set(build.KERNEL_SOURCES["meshraster"])
    assert len(build.source_digest("meshraster")) == 16
    # the pinned neighbours keep their layouts
    assert C.sizeof(_lib.MeshOrient) == lib.nudf_meshorient_struct_size()


def test_launchers_refuse_bad_sizes_without_a_gpu():
    """the size checks are host code: no kernel is launched for a refused or an empty descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    ok = dict(n_faces=4, n_verts=8, n_views=2, H=3, W=5)
    for bad in (dict(n_faces=1 << 31), dict(n_verts=1 << 31), dict(n_faces=-1), dict(n_verts=-1), dict(n_views=-1),
                dict(n_entries=-1), dict(H=-1), dict(W=-1), dict(n_entries=9),              # more entries than (view, face)
                dict(H=1 << 16, W=1 << 15),                                                  # H * W = 2^31
                dict(n_views=1 << 10, H=1 << 15, W=1 << 15),                                 # n_views * H * W = 2^40
                dict(n_views=1 << 20, n_faces=1 << 20), dict(n_views=1 << 20, n_verts=1 << 20)):
        d = _lib.MeshRaster(**{**ok, **bad})
        for e in ENTRIES:
            assert getattr(lib, "nudf_meshraster_" + e)(C.byref(d), None) != 0, (bad, e)
            assert b"nudf_meshraster_" + e.encode() in lib.nudf_last_error()
    d = _lib.MeshRaster(**{**ok, "n_verts": 1 << 31})
    assert lib.nudf_meshraster_project(C.byref(d), None) != 0 and b"2^31" in lib.nudf_last_error()
    # an image of no pixels is refused as soon as there is something to do per view
    for hw in (dict(H=0), dict(W=0)):
        d = _lib.MeshRaster(**{**ok, **hw, "n_entries": 1})
        for e in ENTRIES:
            if e != "project":
                assert getattr(lib, "nudf_meshraster_" + e)(C.byref(d), None) != 0, (hw, e)
                assert b"H and W must be >= 1" in lib.nudf_last_error()
    empty = _lib.MeshRaster()
    for e in ENTRIES:
        assert getattr(lib, "nudf_meshraster_" + e)(C.byref(empty), None) == 0, e
    # nothing to do for this entry point, whatever the other counts say
    d = _lib.MeshRaster(n_faces=4, n_verts=8, H=3, W=5)                  # no views
    for e in ("project", "bounds", "draw_small", "draw_large", "resolve", "visible"):
        assert getattr(lib, "nudf_meshraster_" + e)(C.byref(d), None) == 0, e
    d = _lib.MeshRaster(n_views=2, H=3, W=5, n_faces=4)                  # no vertices, no entries
    for e in ("project", "draw_small", "draw_large", "visible", "colour"):
        assert getattr(lib, "nudf_meshraster_" + e)(C.byref(d), None) == 0, e
    d = _lib.MeshRaster(n_views=2, H=3, W=5, n_verts=8)                  # no faces
    assert lib.nudf_meshraster_bounds(C.byref(d), None) == 0
