"""CPU: the ctypes mirror of NudfMeshUDFSparse (neuraludf_amd/_lib.py) against a C compile of include/nudf.h -- field
names, offsets and size --, the exports, the launchers' host-side size checks and the Python API's ValueErrors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("classify", "edges", "emit", "vertices")


def test_sparse_struct_matches_the_header(tmp_path):
    from neuraludf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nudf.h")).read()
    body = re.search(r"typedef struct NudfMeshUDFSparse \{(.*?)\} NudfMeshUDFSparse;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_0-9]+", d)[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.MeshUDFSparse._fields_]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this box")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nudf.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(NudfMeshUDFSparse));']
    lines += ['  printf("%s %%zu\\n", offsetof(NudfMeshUDFSparse, %s));' % (n, n) for n in names]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.MeshUDFSparse)
    for n in names:
        assert int(got[n]) == getattr(_lib.MeshUDFSparse, n).offset, n


def test_exports_and_struct_size():
    from neuraludf_amd import build, _lib
    build.build()
    lib = _lib.lib()
    for s in ["nudf_meshudf_sparse_struct_size"] + ["nudf_meshudf_sparse_" + e for e in ENTRY]:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.nudf_meshudf_sparse_struct_size() == C.sizeof(_lib.MeshUDFSparse)
    assert "meshudf_sparse.hip" in build.SOURCES
    for k in ("meshudf", "meshudf_sparse"):
        assert "csrc/meshudf_cell.h" in build.KERNEL_SOURCES[k] and len(build.source_digest(k)) == 16


def test_launchers_refuse_bad_sizes_without_a_gpu():
    """the size checks are host code: no kernel is launched for a refused or an empty descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    good = dict(N=96, B=8, nb=12, n_blocks=0)
    for bad in (dict(N=2), dict(N=4097, nb=512), dict(B=5), dict(B=16, nb=6), dict(nb=11), dict(n_blocks=-1),
                dict(n_blocks=12 ** 3 + 1)):
        d = _lib.MeshUDFSparse(**{**good, **bad})
        for e in ENTRY:
            assert getattr(lib, "nudf_meshudf_sparse_" + e)(C.byref(d), None) != 0, (bad, e)
        assert b"nudf_meshudf_sparse" in lib.nudf_last_error()
    for ok in (good, dict(N=4096, B=4, nb=1024, n_blocks=0), dict(N=5, B=8, nb=1, n_blocks=0)):
        d = _lib.MeshUDFSparse(**ok)
        for e in ENTRY:
            assert getattr(lib, "nudf_meshudf_sparse_" + e)(C.byref(d), None) == 0, (ok, e)


def test_python_value_errors():
    from neuraludf_amd import meshing
    import meshudf_sparse_ref as S
    f = S.Field(S.sphere_udf)
    assert (meshing.SPARSE_MIN_N, meshing.SPARSE_MAX_N, meshing.MAX_N) == (3, 4096, 1024)
    for kw in (dict(block=2), dict(block=16), dict(block=8.5), dict(lipschitz=0.0), dict(lipschitz=-1.0),
               dict(lipschitz=float("inf")), dict(lipschitz=float("nan")), dict(lipschitz="2")):
        with pytest.raises(ValueError):
            meshing.udf_sparse_grid(f, 17, device="cpu", **kw)
    for n in (2, 4097):
        with pytest.raises(ValueError):
            meshing.udf_sparse_grid(f, n, device="cpu")
        with pytest.raises(ValueError):
            meshing.extract_udf_mesh(f, n, sparse=True)
    with pytest.raises(ValueError):
        meshing.extract_udf_mesh(f, 17, sparse=True, block=3)
    with pytest.raises(ValueError):
        meshing.udf_marching_cubes_sparse((None, None))
    e = torch.zeros(0)
    g = meshing.SparseUDFGrid(1025, 8, 128, *S.BOX, e, e.long(), e.int(), e.view(0, 729), e.view(0, 729, 3))
    with pytest.raises(ValueError):
        g.to_dense()
    g = meshing.udf_sparse_grid(f, 33, block=4, lipschitz=1.05, device="cpu")
    U, G = g.to_dense()
    assert U.shape == (33, 33, 33) and G.shape == (33, 33, 33, 3) and bool(torch.isinf(U).any()) and bool((U < 1).any())
