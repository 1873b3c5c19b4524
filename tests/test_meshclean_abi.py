"""CPU: the ctypes mirror of NudfMeshTopo (neuraludf_amd/_lib.py) against a C compile of include/nudf.h -- field names,
offsets and size -- and the version the header's new block raised the library to."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_meshtopo_struct_matches_the_header(tmp_path):
    from neuraludf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nudf.h")).read()
    body = re.search(r"typedef struct NudfMeshTopo \{(.*?)\} NudfMeshTopo;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_0-9]+", d)[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.MeshTopo._fields_]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this box")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nudf.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(NudfMeshTopo));']
    lines += ['  printf("%s %%zu\\n", offsetof(NudfMeshTopo, %s));' % (n, n) for n in names]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.MeshTopo)
    for n in names:
        assert int(got[n]) == getattr(_lib.MeshTopo, n).offset, n


def test_version_108_and_exports():
    from neuraludf_amd import build, _lib
    build.build()
    lib = _lib.lib()
    assert lib.nudf_version() == _lib.ABI_VERSION == 108
    for s in ("nudf_meshtopo_edges", "nudf_meshtopo_fill_count", "nudf_meshtopo_fill_emit", "nudf_meshtopo_smooth",
              "nudf_meshtopo_cc_hook", "nudf_meshtopo_cc_jump", "nudf_meshtopo_views"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert "meshtopo.hip" in build.SOURCES


def test_launchers_refuse_bad_sizes_without_a_gpu():
    """the size checks are host code: no kernel is launched for a refused or an empty descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    d = _lib.MeshTopo(n_faces=4, n_verts=1 << 31, n_edges=3)
    assert lib.nudf_meshtopo_edges(C.byref(d), None) != 0 and b"2^31" in lib.nudf_last_error()
    d = _lib.MeshTopo(n_faces=4, n_verts=8, n_bverts=3, max_loop=5)
    assert lib.nudf_meshtopo_fill_count(C.byref(d), None) != 0
    assert lib.nudf_meshtopo_fill_emit(C.byref(d), None) != 0
    d = _lib.MeshTopo(n_verts=8, n_views=1, H=0, W=4)
    assert lib.nudf_meshtopo_views(C.byref(d), None) != 0
    e = _lib.MeshTopo(max_loop=4, H=1, W=1)
    for name in ("edges", "fill_count", "fill_emit", "smooth", "cc_hook", "cc_jump", "views"):
        assert getattr(lib, "nudf_meshtopo_" + name)(C.byref(e), None) == 0
