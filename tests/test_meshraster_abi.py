"""CPU: the rasteriser's place in the build and the launchers' host-side size checks.  (The ctypes mirror of
NudfMeshRaster, its size in the library, the library version and the exports: tests/test_abi.py.)"""
import ctypes as C

ENTRIES = ("project", "bounds", "draw_small", "draw_large", "resolve", "visible", "colour")


def test_build_lists_the_sources():
    from neuraludf_amd import build
    build.build()
    assert "meshraster.hip" in build.SOURCES
    assert {"csrc/meshraster.hip", "csrc/meshraster_pixel.h"} <= set(build.KERNEL_SOURCES["meshraster"])
    assert len(build.source_digest("meshraster")) == 16


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
