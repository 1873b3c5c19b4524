"""CPU: the simplification kernels' place in the build and the launchers' host-side checks.  (The ctypes mirror of
NudfMeshTopo with the sp_ fields, its size in the library, the library version and the exports: tests/test_abi.py.)"""
import ctypes as C
import math

ENTRIES = ("keys", "place", "faces")


def _desc(**kw):
    """a descriptor that would launch every entry point: counts, a grid, a cell and the place parameters, no buffers"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, n_clusters=2, sp_cell=0.5, sp_lambda=1e-3, sp_boundary_weight=1.0)
    grid, origin = kw.pop("grid", (3, 3, 3)), kw.pop("origin", (0.0, 0.0, 0.0))
    args.update(kw)
    d = _lib.MeshTopo(**args)
    for x in range(3):
        d.sp_grid[x], d.sp_origin[x] = grid[x], origin[x]
    return d


def test_build_lists_the_source():
    from neuraludf_amd import build
    build.build()
    assert "meshsimplify.hip" in build.SOURCES
    assert "csrc/meshsimplify.hip" in build.KERNEL_SOURCES["meshsimplify"]
    digest = build.source_digest("meshsimplify")
    assert len(digest) == 16 and int(digest, 16) >= 0


def test_launchers_refuse_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    everywhere = (dict(n_verts=1 << 31), dict(n_verts=-1), dict(n_faces=-1), dict(grid=(3, (1 << 20) + 1, 3)),
                  dict(grid=(3, 3, -1)), dict(sp_attr_width=-1), dict(n_clusters=9), dict(n_clusters=-1))
    for bad in everywhere:
        for e in ENTRIES:
            assert getattr(lib, "nudf_meshsimplify_" + e)(C.byref(_desc(**bad)), None) != 0, (bad, e)
            assert b"nudf_meshsimplify_" + e.encode() in lib.nudf_last_error()
    assert lib.nudf_meshsimplify_keys(C.byref(_desc(n_verts=1 << 31)), None) != 0 and b"2^31" in lib.nudf_last_error()
    assert lib.nudf_meshsimplify_keys(C.byref(_desc(grid=(1 << 21, 1, 1))), None) != 0 and b"2^20" in lib.nudf_last_error()
    # the entry points that compute keys need a cell and a grid to compute them with
    for bad in (dict(sp_cell=0.0), dict(sp_cell=-1.0), dict(sp_cell=math.inf), dict(sp_cell=math.nan),
                dict(grid=(3, 0, 3)), dict(origin=(0.0, math.nan, 0.0)), dict(origin=(math.inf, 0.0, 0.0))):
        for e in ("keys", "place"):
            assert getattr(lib, "nudf_meshsimplify_" + e)(C.byref(_desc(**bad)), None) != 0, (bad, e)
            assert b"nudf_meshsimplify_" + e.encode() in lib.nudf_last_error()
    for bad in (dict(sp_lambda=0.0), dict(sp_lambda=math.nan), dict(sp_boundary_weight=-1.0), dict(sp_placement=2)):
        assert lib.nudf_meshsimplify_place(C.byref(_desc(**bad)), None) != 0, bad
        assert b"NULL" not in lib.nudf_last_error()
    # sizes and parameters in order, but no buffers: refused before any launch
    for e in ENTRIES:
        assert getattr(lib, "nudf_meshsimplify_" + e)(C.byref(_desc()), None) != 0, e
        assert b"NULL" in lib.nudf_last_error()


def test_launchers_accept_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    empty = _lib.MeshTopo()
    for e in ENTRIES:
        assert getattr(lib, "nudf_meshsimplify_" + e)(C.byref(empty), None) == 0, e
    # nothing to do for this entry point, whatever the other counts say
    assert lib.nudf_meshsimplify_keys(C.byref(_desc(n_verts=0, n_clusters=0)), None) == 0
    assert lib.nudf_meshsimplify_place(C.byref(_desc(n_clusters=0)), None) == 0
    assert lib.nudf_meshsimplify_faces(C.byref(_desc(n_faces=0)), None) == 0


def test_mesh_topo_grew_at_its_end_only():
    """the clean-up's fields keep their offsets: the simplification's were appended"""
    from neuraludf_amd import _lib
    names = [f[0] for f in _lib.MeshTopo._fields_]
    first = names.index("sp_key")
    assert names[first - 1] == "pad_" and all(n.startswith("sp_") or n == "n_clusters" for n in names[first:])
    assert _lib.MeshTopo.sp_key.offset == _lib.MeshTopo.pad_.offset + 4 and _lib.MeshTopo.sp_key.offset % 8 == 0
