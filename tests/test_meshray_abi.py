"""CPU: the ray-casting kernel's place in the build and the launcher's host-side checks.  (The ctypes mirror of
NudfPointCloud with the ray fields, its size in the library and the export: tests/test_abi.py.)"""
import ctypes as C
import math

BUFFERS = ("verts", "faces", "query_idx", "cell_start", "cell_count", "hash_key", "hash_row", "dist", "idx",
           "md_cell_face", "md_bary", "md_ray_o", "md_ray_d", "md_count")
RAY_FIELDS = ["md_ray_o", "md_ray_d", "md_t_min", "md_t_max", "md_ray_window", "md_mode", "md_pad_", "md_count"]


def _desc(buffers=True, **kw):
    """a descriptor the entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, n_query=5, cell=0.5, md_n_refs=12, n_cells=3, hash_cap=8, md_t_min=0.0,
                md_t_max=math.inf, md_mode=0)
    if buffers:
        args.update({b: 4096 for b in BUFFERS})
    grid = kw.pop("grid", (3, 3, 3))
    args.update(kw)
    d = _lib.PointCloud(**args)
    d.grid[:] = grid
    return d


def _refused(lib, d, word):
    assert lib.nudf_pc_raycast(C.byref(d), None) != 0, word
    err = lib.nudf_last_error()
    assert b"nudf_pc_raycast" in err and word in err, (word, err)


def test_build_lists_the_source():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshray.hip" in build.SOURCES
    assert "csrc/meshray.hip" in build.KERNEL_SOURCES["meshray"]
    digest = build.source_digest("meshray")
    assert len(digest) == 16 and int(digest, 16) >= 0
    assert "nudf_pc_raycast" in _lib.SIGNATURES and "nudf_pc_raycast" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "nudf_pc_raycast")


def test_launcher_refuses_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf)):
        _refused(lib, _desc(**bad), b"cell")
    for bad in (dict(grid=(3, 0, 3)), dict(grid=(3, 3, (1 << 21) + 1)), dict(grid=(-1, 3, 3))):
        _refused(lib, _desc(**bad), b"grid")
    for bad in (6, 4, 0):
        _refused(lib, _desc(hash_cap=bad), b"hash_cap")
    for n in ("n_query", "n_faces", "n_verts"):
        _refused(lib, _desc(**{n: 1 << 31}), b"2^31")
    for bad in (3, -1, 17):
        _refused(lib, _desc(md_mode=bad), b"mode")
    _refused(lib, _desc(md_t_min=math.nan), b"t_min")
    _refused(lib, _desc(md_t_min=1.0, md_t_max=0.5), b"t_max")
    _refused(lib, _desc(md_t_max=math.nan), b"t_max")
    _refused(lib, _desc(buffers=False), b"NULL")
    for b in ("verts", "faces", "query_idx", "cell_start", "cell_count", "hash_key", "hash_row", "md_cell_face", "md_ray_o",
              "md_ray_d", "dist", "idx", "md_bary"):
        _refused(lib, _desc(**{b: None}), b"NULL")
    for mode in (1, 2):
        _refused(lib, _desc(md_mode=mode, md_count=None), b"NULL")
    # the largest grid is accepted as far as the host checks go: the refusal that is left is the missing buffers
    _refused(lib, _desc(buffers=False, grid=(1 << 21, 1, 1 << 21)), b"NULL")


def test_launcher_accepts_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    assert lib.nudf_pc_raycast(C.byref(_lib.PointCloud()), None) == 0
    # nothing to do, whatever the other fields say
    assert lib.nudf_pc_raycast(C.byref(_desc(n_query=0, md_mode=9, cell=-1.0, buffers=False)), None) == 0


def test_point_cloud_grew_at_its_end_only():
    """the fields of the Chamfer evaluation and of the point-to-mesh distance keep their offsets: the ray fields were
    appended, and everything after md_ref_n still carries the md_ prefix"""
    from neuraludf_amd import _lib
    names = [f[0] for f in _lib.PointCloud._fields_]
    assert names[names.index("md_bary") + 1:] == RAY_FIELDS
    assert _lib.PointCloud.md_ray_o.offset == _lib.PointCloud.md_bary.offset + 8
    assert all(n.startswith("md_") for n in names[names.index("md_ref_n"):])
    assert _lib.PointCloud.md_count.offset + 8 == C.sizeof(_lib.PointCloud)
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()
