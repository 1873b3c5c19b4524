"""CPU: the sparse MeshUDF mesher's place in the build, the launchers' host-side size checks and the Python API's
ValueErrors.  (The ctypes mirror of NudfMeshUDFSparse, its size in the library and the exports: tests/test_abi.py.)"""
import ctypes as C

import pytest
import torch

ENTRY = ("classify", "edges", "emit", "vertices")


def test_build_lists_the_sources():
    from neuraludf_amd import build
    build.build()
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
