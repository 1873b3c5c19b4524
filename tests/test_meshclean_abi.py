"""CPU: the mesh clean-up kernels' place in the build and the launchers' host-side size checks.  (The ctypes mirror of
NudfMeshTopo, the library version and the exports: tests/test_abi.py.)"""
import ctypes as C


def test_build_lists_the_sources():
    from neuraludf_amd import build
    build.build()
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
