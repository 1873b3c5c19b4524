"""CPU: the ctypes mirror of NudfMeshOrient (neuraludf_amd/_lib.py) against a C compile of include/nudf.h -- field names,
offsets and size --, the exports, the struct size the loader checks, the launchers' host-side size checks, and the
library version, which this block leaves alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hook", "jump", "check", "outward", "normals")


def test_meshorient_struct_matches_the_header(tmp_path):
    from neuraludf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nudf.h")).read()
    body = re.search(r"typedef struct NudfMeshOrient \{(.*?)\} NudfMeshOrient;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", d)[-1] for d in body.split(";") if d.strip()]       # `origin[3]` -> origin
    assert names == [f[0] for f in _lib.MeshOrient._fields_]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this box")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nudf.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(NudfMeshOrient));']
    lines += ['  printf("%s %%zu\\n", offsetof(NudfMeshOrient, %s));' % (n, n) for n in names]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.MeshOrient)
    for n in names:
        assert int(got[n]) == getattr(_lib.MeshOrient, n).offset, n


def test_exports_struct_size_and_version():
    from neuraludf_amd import build, _lib
    build.build()
    lib = _lib.lib()
    assert lib.nudf_version() == _lib.ABI_VERSION == 108
    for s in ["nudf_meshorient_struct_size"] + ["nudf_meshorient_" + e for e in ENTRIES]:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.nudf_meshorient_struct_size() == C.sizeof(_lib.MeshOrient)
    assert "meshorient.hip" in build.SOURCES and "meshtopo.hip" in build.SOURCES
    assert "csrc/meshorient.hip" in build.KERNEL_SOURCES["meshorient"]
    assert len(build.source_digest("meshorient")) == 16


def test_launchers_refuse_bad_sizes_without_a_gpu():
    """the size checks are host code: no kernel is launched for a refused or an empty descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad in (dict(n_faces=4, n_verts=1 << 31), dict(n_faces=-1), dict(n_verts=-1), dict(n_faces=4, n_medges=-1),
                dict(n_faces=4, n_verts=8, n_medges=7), dict(n_faces=4, n_verts=8, n_comps=5),
                dict(n_faces=4, n_verts=8, n_comps=-1), dict(n_faces=1 << 36, n_verts=8)):
        d = _lib.MeshOrient(**bad)
        for e in ENTRIES:
            assert getattr(lib, "nudf_meshorient_" + e)(C.byref(d), None) != 0, (bad, e)
            assert b"nudf_meshorient_" + e.encode() in lib.nudf_last_error()
    d = _lib.MeshOrient(n_faces=4, n_verts=1 << 31)
    assert lib.nudf_meshorient_hook(C.byref(d), None) != 0 and b"2^31" in lib.nudf_last_error()
    empty = _lib.MeshOrient()
    for e in ENTRIES:
        assert getattr(lib, "nudf_meshorient_" + e)(C.byref(empty), None) == 0, e
    # nothing to do for this entry point, whatever the other counts say
    d = _lib.MeshOrient(n_faces=4, n_verts=8)                # no manifold edges, no components
    for e in ("hook", "check", "outward"):
        assert getattr(lib, "nudf_meshorient_" + e)(C.byref(d), None) == 0, e
    d = _lib.MeshOrient(n_faces=0, n_verts=0)
    for e in ("jump", "normals"):
        assert getattr(lib, "nudf_meshorient_" + e)(C.byref(d), None) == 0, e
