"""CPU: the face-orientation kernels' place in the build and the launchers' host-side size checks.  (The ctypes mirror of
NudfMeshOrient, its size in the library, the library version and the exports: tests/test_abi.py.)"""
import ctypes as C

ENTRIES = ("hook", "jump", "check", "outward", "normals")


def test_build_lists_the_sources():
    from neuraludf_amd import build
    build.build()
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
