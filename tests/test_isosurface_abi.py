"""CPU: the level-set mesher's place in the build, the launchers' host-side size checks, the Python API's ValueErrors and
the block selection of iso_sparse_grid against the numpy restatement (tests/isosurface_ref.py).  (The ctypes mirrors of
NudfIsoSurface / NudfIsoSurfaceSparse, their sizes in the library and the exports: tests/test_abi.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import isosurface_ref as I

DENSE = ("classify", "emit", "vertices")
SPARSE = ("classify", "edges", "emit", "vertices")


def test_build_lists_the_sources():
    from neuraludf_amd import build
    build.build()
    assert "isosurface.hip" in build.SOURCES
    for f in ("csrc/isosurface.hip", "csrc/isosurface_cell.h", "csrc/mc_tables.inc"):
        assert f in build.KERNEL_SOURCES["isosurface"]
    assert len(build.source_digest("isosurface")) == 16


def test_launchers_refuse_bad_sizes_without_a_gpu():
    """the size checks are host code: no kernel is launched for a refused or an empty descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for n in (2, 0, -1, 1025):
        d = _lib.IsoSurface(N=n)
        for e in DENSE:
            assert getattr(lib, "nudf_isosurface_" + e)(C.byref(d), None) != 0, (n, e)
        assert b"nudf_isosurface" in lib.nudf_last_error()
    for n in (3, 1024):                                      # emit and vertices of an empty descriptor launch nothing
        d = _lib.IsoSurface(N=n, n_cells=0, n_edges=0)
        for e in ("emit", "vertices"):
            assert getattr(lib, "nudf_isosurface_" + e)(C.byref(d), None) == 0, (n, e)
    good = dict(N=96, B=8, nb=12, n_blocks=0)
    for bad in (dict(N=2), dict(N=4097, nb=512), dict(B=5), dict(B=16, nb=6), dict(nb=11), dict(n_blocks=-1),
                dict(n_blocks=12 ** 3 + 1)):
        d = _lib.IsoSurfaceSparse(**{**good, **bad})
        for e in SPARSE:
            assert getattr(lib, "nudf_isosurface_sparse_" + e)(C.byref(d), None) != 0, (bad, e)
        assert b"nudf_isosurface_sparse" in lib.nudf_last_error()
    for ok in (good, dict(N=4096, B=4, nb=1024, n_blocks=0), dict(N=5, B=8, nb=1, n_blocks=0)):
        d = _lib.IsoSurfaceSparse(**ok)
        for e in SPARSE:
            assert getattr(lib, "nudf_isosurface_sparse_" + e)(C.byref(d), None) == 0, (ok, e)


def test_python_value_errors():
    from neuraludf_amd import meshing
    from neuraludf_amd.models import udf_renderer_blending as rb
    F = torch.zeros((4, 4, 4))
    for bad in (F.double(), F.numpy(), F, F[:3], F[0], torch.zeros((4, 4, 4, 1))):      # dtype, type, CPU, shape
        with pytest.raises(ValueError):
            meshing.iso_marching_cubes(bad, 0.0, *I.BOX)
    for level in (float("nan"), float("inf"), -float("inf"), "0", None, True, 1e39):
        with pytest.raises(ValueError):
            meshing.iso_sparse_grid(I.sphere_sdf, 17, level, *I.BOX, device="cpu")
        with pytest.raises(ValueError):
            meshing.extract_iso_mesh(I.sphere_sdf, 17, level, device="cpu")
    for kw in (dict(block=2), dict(block=16), dict(block=8.5), dict(lipschitz=0.0), dict(lipschitz=-1.0),
               dict(lipschitz=float("inf")), dict(lipschitz=float("nan")), dict(lipschitz="2")):
        with pytest.raises(ValueError):
            meshing.iso_sparse_grid(I.sphere_sdf, 17, 0.0, *I.BOX, device="cpu", **kw)
        with pytest.raises(ValueError):
            meshing.extract_iso_mesh(I.sphere_sdf, 17, sparse=True, device="cpu", **kw)
    for n in (2, 4097):
        with pytest.raises(ValueError):
            meshing.iso_sparse_grid(I.sphere_sdf, n, 0.0, *I.BOX, device="cpu")
    for n in (2, 1025):
        with pytest.raises(ValueError):
            meshing.extract_iso_mesh(I.sphere_sdf, n, device="cpu")
    with pytest.raises(ValueError):
        meshing.iso_marching_cubes_sparse(None, 0.0)
    g = meshing.iso_sparse_grid(I.sphere_sdf, 17, 0.0, *I.BOX, block=4, device="cpu")
    with pytest.raises(ValueError):
        meshing.iso_marching_cubes_sparse(g, float("nan"))
    with pytest.raises(ValueError):                          # a UDF grid is not a field grid
        meshing.iso_marching_cubes_sparse(meshing.SparseUDFGrid(17, 4, 4, *I.BOX, g.axes, g.blocks, g.block_slot, g.F, None),
                                          0.0)
    g.N = 1025
    with pytest.raises(ValueError):
        g.to_dense()
    with pytest.raises(ValueError, match="mesher"):
        rb.extract_geometry(*I.BOX, 17, 0.0, I.sphere_sdf, "cpu", mesher="skimage")


@pytest.mark.parametrize("level, lipschitz", [(0.0, 1.05), (0.13, 2.0)])
def test_cpu_selection_equals_the_restatement(level, lipschitz):
    from neuraludf_amd import meshing
    n, b = 33, 4
    g = meshing.iso_sparse_grid(I.sphere_sdf, n, level, *I.BOX, block=b, lipschitz=lipschitz, device="cpu")
    lo, hi = I.selection_bounds(*I.BOX, n, level, b, lipschitz)
    assert (lo, hi) == meshing.iso_selection_bounds(*I.BOX, n, level, b, lipschitz) and lo.dtype == hi.dtype == np.float32
    coarse = I.coarse_values(I.sphere_sdf, n, b, *I.BOX)
    np.testing.assert_array_equal(g.coarse.numpy(), coarse)
    blocks = I.select(coarse, n, b, lo, hi)
    np.testing.assert_array_equal(g.blocks.numpy(), blocks)
    assert (g.N, g.B, g.nb, g.n_coarse) == (n, b, 8, 9 ** 3) and 0 < g.n_blocks == len(blocks) < 8 ** 3
    # every cut cell of the dense grid lies in a selected block, and the bricks hold the dense values
    F = I.grid_values(I.sphere_sdf, n, *I.BOX)
    assert I.uncovered_cut_cells(F.numpy(), level, blocks, b) == 0
    D = g.to_dense()
    held = torch.isfinite(D)
    assert int(held.sum()) == g.n_queried and torch.equal(D[held], F[held])
    slot = g.block_slot.numpy()
    assert slot.dtype == np.int32 and (slot[blocks] == np.arange(len(blocks))).all() and (slot >= 0).sum() == len(blocks)


def test_nan_corner_never_selects():
    from neuraludf_amd import meshing
    n, b = 17, 4

    def fn(p):
        f = I.sphere_sdf(p)
        return torch.where((p == 0).all(-1), torch.full_like(f, float("nan")), f)      # the centre node is a coarse node
    g = meshing.iso_sparse_grid(fn, n, -0.7, *I.BOX, block=b, lipschitz=1.05, device="cpu")
    coarse = g.coarse.numpy()
    assert np.isnan(coarse).sum() == 1
    blocks = I.select(coarse, n, b, *I.selection_bounds(*I.BOX, n, -0.7, b, 1.05))
    np.testing.assert_array_equal(g.blocks.numpy(), blocks)
    clean = meshing.iso_sparse_grid(I.sphere_sdf, n, -0.7, *I.BOX, block=b, lipschitz=1.05, device="cpu")
    assert clean.n_blocks == 8 and g.n_blocks == 0           # the eight blocks round the centre all hold the NaN corner
