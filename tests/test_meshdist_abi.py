"""CPU: the point-to-mesh kernels' place in the build, the library version and the launchers' host-side checks.  (The
ctypes mirror of NudfPointCloud with the md_ fields, its size in the library and the exports: tests/test_abi.py.)"""
import ctypes as C
import math

ENTRIES = ("tribin_count", "tribin_emit", "closest")
BUFFERS = ("verts", "faces", "query", "query_idx", "cell_start", "cell_count", "hash_key", "hash_row", "dist", "idx",
           "md_ref_n", "md_ref_off", "md_ref_key", "md_ref_face", "md_cell_face", "md_point", "md_bary")


def _desc(buffers=True, **kw):
    """a descriptor every entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, n_query=5, cell=0.5, cap=100, md_n_refs=12, n_cells=3, hash_cap=8, bound=math.inf)
    if buffers:
        args.update({b: 4096 for b in BUFFERS})
    grid = kw.pop("grid", (3, 3, 3))
    args.update(kw)
    d = _lib.PointCloud(**args)
    d.grid[:] = grid
    return d


def _refused(lib, entry, d, word=None):
    assert getattr(lib, "nudf_pc_" + entry)(C.byref(d), None) != 0, entry
    err = lib.nudf_last_error()
    assert b"nudf_pc_" + entry.encode() in err, err
    if word is not None:
        assert word in err, err


def test_build_lists_the_source_and_the_version():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshdist.hip" in build.SOURCES
    assert "csrc/meshdist.hip" in build.KERNEL_SOURCES["meshdist"]
    digest = build.source_digest("meshdist")
    assert len(digest) == 16 and int(digest, 16) >= 0
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()


def test_launchers_refuse_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf)):
            _refused(lib, e, _desc(**bad), b"cell")
        for bad in (dict(grid=(3, 0, 3)), dict(grid=(3, 3, (1 << 21) + 1)), dict(grid=(-1, 3, 3))):
            _refused(lib, e, _desc(**bad), b"grid")
        _refused(lib, e, _desc(n_verts=1 << 31), b"2^31")
        _refused(lib, e, _desc(n_faces=1 << 31), b"2^31")
        _refused(lib, e, _desc(buffers=False), b"NULL")
        _refused(lib, e, _desc(verts=None), b"NULL")
    for e in ("tribin_count", "tribin_emit"):
        _refused(lib, e, _desc(cap=-1), b"cap")
        _refused(lib, e, _desc(cap=(1 << 40) + 1), b"cap")
        _refused(lib, e, _desc(md_ref_n=None), b"NULL")
    _refused(lib, "tribin_emit", _desc(md_ref_key=None), b"NULL")
    _refused(lib, "closest", _desc(n_query=1 << 31), b"2^31")
    for bad in (0.0, -1.0, math.nan):
        _refused(lib, "closest", _desc(bound=bad), b"bound")
    _refused(lib, "closest", _desc(hash_cap=6), b"hash_cap")
    _refused(lib, "closest", _desc(hash_cap=4), b"hash_cap")
    _refused(lib, "closest", _desc(md_bary=None), b"NULL")
    _refused(lib, "closest", _desc(md_cell_face=None), b"NULL")
    # the largest grid is accepted as far as the host checks go: the refusal that is left is the missing buffers
    _refused(lib, "closest", _desc(buffers=False, grid=(1 << 21, 1, 1 << 21)), b"NULL")


def test_launchers_accept_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    empty = _lib.PointCloud()
    for e in ENTRIES:
        assert getattr(lib, "nudf_pc_" + e)(C.byref(empty), None) == 0, e
    # nothing to do for this entry point, whatever the other fields say
    assert lib.nudf_pc_tribin_count(C.byref(_desc(n_faces=0, cell=-1.0)), None) == 0
    assert lib.nudf_pc_tribin_emit(C.byref(_desc(n_faces=0, buffers=False)), None) == 0
    assert lib.nudf_pc_closest(C.byref(_desc(n_query=0, bound=-1.0)), None) == 0


def test_point_cloud_grew_at_its_end_only():
    """the Chamfer evaluation's fields keep their offsets: the point-to-mesh fields were appended"""
    from neuraludf_amd import _lib
    names = [f[0] for f in _lib.PointCloud._fields_]
    first = names.index("md_ref_n")
    assert names[first - 1] == "idx" and all(n.startswith("md_") for n in names[first:])
    assert _lib.PointCloud.md_ref_n.offset == _lib.PointCloud.idx.offset + 8
