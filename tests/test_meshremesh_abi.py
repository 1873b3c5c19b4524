"""CPU: the remeshing kernels' place in the build, the launchers' host-side checks, and the way NudfMeshTopo grew: after
the hole closing's fields only, under the same ABI version.  (The ctypes mirror against the header, its size in the library
and the exports: tests/test_abi.py; the prefixes of the tail: tests/test_meshsubdiv_abi.py, tests/test_meshhole_abi.py.)"""
import ctypes as C
import math
import os
import re

ENTRIES = ("collapse_check", "vertex_min", "collapse_apply", "flip_check", "flip_apply", "relax")
BUFFERS = ("faces", "edges", "he_edge", "he_id", "edge_start", "edge_key", "pos", "nbr_off", "nbr", "sp_sd_ring_off", "sp_sd_ring",
           "sp_sd_vclass", "sp_sd_hf_rm_corner_off", "sp_sd_hf_rm_corner", "sp_sd_hf_rm_vedge_off", "sp_sd_hf_rm_vedge",
           "sp_sd_hf_rm_status", "sp_sd_hf_rm_keep", "sp_sd_hf_rm_gone", "sp_sd_hf_rm_gain", "sp_sd_hf_rm_ab", "sp_sd_hf_rm_rank",
           "sp_sd_hf_rm_best_in", "sp_sd_hf_rm_remap", "sp_sd_hf_rm_pos_out", "sp_sd_hf_rm_faces_out", "sp_sd_hf_rm_win")
READS = dict(
    collapse_check=("faces", "edges", "he_id", "edge_start", "pos", "sp_sd_vclass", "nbr_off", "nbr", "sp_sd_ring_off",
                    "sp_sd_ring", "sp_sd_hf_rm_corner_off", "sp_sd_hf_rm_corner", "sp_sd_hf_rm_status", "sp_sd_hf_rm_keep",
                    "sp_sd_hf_rm_gone"),
    collapse_apply=("edges", "pos", "sp_sd_vclass", "sp_sd_hf_rm_status", "sp_sd_hf_rm_rank", "sp_sd_hf_rm_keep", "sp_sd_hf_rm_gone",
                    "sp_sd_hf_rm_best_in", "sp_sd_hf_rm_remap", "sp_sd_hf_rm_pos_out", "sp_sd_hf_rm_win"),
    flip_check=("faces", "edges", "he_id", "edge_start", "edge_key", "pos", "sp_sd_vclass", "sp_sd_ring_off", "sp_sd_ring",
                "sp_sd_hf_rm_status", "sp_sd_hf_rm_gain", "sp_sd_hf_rm_ab"),
    flip_apply=("faces", "edges", "he_id", "edge_start", "sp_sd_hf_rm_status", "sp_sd_hf_rm_rank", "sp_sd_hf_rm_ab",
                "sp_sd_hf_rm_best_in", "sp_sd_hf_rm_faces_out", "sp_sd_hf_rm_win"),
    relax=("pos", "sp_sd_hf_rm_pos_out", "sp_sd_vclass", "sp_sd_ring_off", "sp_sd_ring", "sp_sd_hf_rm_vedge_off", "sp_sd_hf_rm_vedge",
           "edges", "faces"))
MIN_READS = {0: ("sp_sd_hf_rm_best_out", "sp_sd_hf_rm_status", "sp_sd_hf_rm_rank", "sp_sd_hf_rm_vedge_off", "sp_sd_hf_rm_vedge"),
             1: ("sp_sd_hf_rm_best_out", "sp_sd_hf_rm_best_in", "sp_sd_ring_off", "sp_sd_ring"),
             2: ("sp_sd_hf_rm_best_out", "sp_sd_hf_rm_status", "sp_sd_hf_rm_rank", "sp_sd_hf_rm_corner_off", "sp_sd_hf_rm_corner",
                 "he_edge")}
# the hole closing's last field and the size of the struct before the remeshing's fields were appended
PARENT_LAST, PARENT_SIZE = "sp_sd_hf_pad_", 712
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nudf.h")


def _desc(buffers=True, **kw):
    """a descriptor every entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=8, n_verts=9, n_edges=16, sp_sd_n_ring=32, sp_sd_n_border=8, sp_sd_hf_rm_n_vedge=32,
                sp_sd_hf_rm_low=0.8, sp_sd_hf_rm_high=1.25, sp_sd_hf_rm_cos_border=0.5, sp_sd_hf_rm_mode=1)
    if buffers:
        args.update({b: 4096 for b in BUFFERS}, sp_sd_hf_rm_best_out=8192)
    args.update(kw)
    return _lib.MeshTopo(**args)


def _call(lib, entry, d):
    return getattr(lib, "nudf_meshremesh_" + entry)(C.byref(d), None)


def _refused(lib, entry, d, word):
    assert _call(lib, entry, d) != 0, (entry, word)
    err = lib.nudf_last_error()
    assert b"nudf_meshremesh_" + entry.encode() in err and word in err, (entry, word, err)


def test_build_lists_the_source():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshremesh.hip" in build.SOURCES
    assert build.KERNEL_SOURCES["meshremesh"] == ["csrc/meshremesh.hip", *build._MESH_COMMON]
    assert len(build.source_digest("meshremesh")) == 16
    text = open(HEADER).read()
    for e in ENTRIES:
        assert "nudf_meshremesh_" + e in _lib.SIGNATURES and "nudf_meshremesh_" + e in _lib.SYMBOLS
        assert hasattr(_lib.lib(), "nudf_meshremesh_" + e)
        assert _lib.SIGNATURES["nudf_meshremesh_" + e][1][0] is C.POINTER(_lib.MeshTopo)
        assert re.search(r"^int nudf_meshremesh_%s\(const NudfMeshTopo\* args, void\* stream\);" % e, text, re.M)
    src = open(os.path.join(os.path.dirname(build.__file__), "csrc", "meshremesh.hip")).read()
    code = [ln for ln in src.splitlines() if ln.strip() and not ln.lstrip().startswith("//")]
    assert code[0] == "#pragma clang fp contract(off)"
    assert "atomic" not in src.replace("no atomics", "")


def test_constants_equal_the_header():
    from neuraludf_amd import _lib, meshclean
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    codes = {k: int(v) for k, v in re.findall(r"\bNUDF_REMESH_(\w+) = (\d+)", text)}
    assert codes == _lib.REMESH and sorted(codes.values()) == list(range(12)) and codes["CANDIDATE"] == 0
    assert meshclean.REMESH_STATUS_NAMES == {v: k.lower() for k, v in codes.items()}
    import meshremesh_ref as ref
    for k, v in codes.items():
        assert getattr(ref, k) == v, k
    assert ref.RING_PASSES == meshclean._REMESH_RING_PASSES == 2


def test_launchers_refuse_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        for bad, word in ((dict(n_faces=-1), b"n_faces"), (dict(n_faces=1 << 31), b"n_faces"), (dict(n_verts=-1), b"n_verts"),
                          (dict(n_verts=1 << 31), b"2^31"), (dict(n_edges=-1), b"n_edges"), (dict(n_edges=25), b"n_edges"),
                          (dict(sp_sd_n_ring=-1), b"sp_sd_n_ring"), (dict(sp_sd_n_border=-1), b"sp_sd_n_border"),
                          (dict(sp_sd_hf_rm_n_vedge=-1), b"sp_sd_hf_rm_n_vedge")):
            _refused(lib, e, _desc(**bad), word)
        _refused(lib, e, _desc(buffers=False), b"NULL")
    for e, reads in READS.items():
        for b in reads:
            _refused(lib, e, _desc(**{b: None}), b"NULL")
            assert b.encode() in lib.nudf_last_error(), (e, b)
    for mode, reads in MIN_READS.items():
        for b in reads:
            _refused(lib, "vertex_min", _desc(sp_sd_hf_rm_mode=mode, **{b: None}), b"NULL")
            assert b.encode() in lib.nudf_last_error(), (mode, b)
    for bad in (-1, 3, 99):
        _refused(lib, "vertex_min", _desc(sp_sd_hf_rm_mode=bad), b"sp_sd_hf_rm_mode")
    _refused(lib, "vertex_min", _desc(sp_sd_hf_rm_mode=1, sp_sd_hf_rm_best_out=4096), b"must differ")
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        _refused(lib, "collapse_check", _desc(sp_sd_hf_rm_low=bad), b"sp_sd_hf_rm_low")
        _refused(lib, "collapse_check", _desc(sp_sd_hf_rm_high=bad), b"sp_sd_hf_rm_high")
    for bad in (1.5, -1.5, math.nan):
        _refused(lib, "collapse_check", _desc(sp_sd_hf_rm_cos_border=bad), b"sp_sd_hf_rm_cos_border")


def test_launchers_accept_what_they_do_not_read():
    """refusals are about the fields an entry point uses: the next one in line is reported"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    # only collapse_check reads the bounds; the apply kernels read no one-ring
    for e in ("collapse_apply", "flip_check", "flip_apply", "relax"):
        _refused(lib, e, _desc(sp_sd_hf_rm_low=math.nan, sp_sd_hf_rm_high=-1.0, sp_sd_hf_rm_cos_border=7.0, sp_sd_hf_rm_mode=9,
                               edges=None), b"NULL")
    _refused(lib, "collapse_apply", _desc(sp_sd_ring_off=None, sp_sd_hf_rm_corner=None, faces=None, sp_sd_hf_rm_win=None),
             b"sp_sd_hf_rm_win")
    # the pass over the one-rings reads neither ranks nor statuses, the pass over the edges no one-ring
    _refused(lib, "vertex_min", _desc(sp_sd_hf_rm_mode=1, sp_sd_hf_rm_status=None, sp_sd_hf_rm_rank=None, sp_sd_ring_off=None),
             b"NULL sp_sd_hf_rm_best_in, sp_sd_ring_off")
    _refused(lib, "vertex_min", _desc(sp_sd_hf_rm_mode=0, sp_sd_ring_off=None, sp_sd_hf_rm_best_in=None, sp_sd_hf_rm_vedge_off=None),
             b"NULL sp_sd_hf_rm_vedge_off")


def test_launchers_accept_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        assert _call(lib, e, _lib.MeshTopo()) == 0, e
    # nothing to do for this entry point, whatever the other fields say
    empty = dict(buffers=False, sp_sd_hf_rm_low=math.nan, sp_sd_hf_rm_high=0.0, sp_sd_hf_rm_mode=9)
    for e in ("collapse_check", "collapse_apply", "flip_check", "flip_apply"):
        assert _call(lib, e, _desc(n_edges=0, **empty)) == 0, e
    for e in ("vertex_min", "relax"):
        assert _call(lib, e, _desc(n_verts=0, **empty)) == 0, e


def test_mesh_topo_grew_after_the_hole_closing_only():
    from neuraludf_amd import _lib
    M = _lib.MeshTopo
    names = [f[0] for f in M._fields_]
    tail = names[names.index(PARENT_LAST) + 1:]
    assert tail and all(n.startswith("sp_sd_hf_rm_") for n in tail)
    assert not any(n.startswith("sp_sd_hf_rm_") for n in names[:names.index(PARENT_LAST) + 1])
    assert getattr(M, tail[0]).offset == getattr(M, PARENT_LAST).offset + 4 == PARENT_SIZE
    assert C.sizeof(M) > PARENT_SIZE and C.sizeof(M) % 8 == 0


def test_version_and_struct_count_are_unchanged():
    from neuraludf_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define NUDF_ABI_VERSION 111$", text, re.M)
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()
    assert len(_lib.MIRRORS) == 31
    version, table = _lib._abi_report(_lib.lib())
    assert version == 111 and len(table) == 31 and table["NudfMeshTopo"] == C.sizeof(_lib.MeshTopo)
    assert _lib._abi_mismatch(version, dict(table, NudfMeshTopo=PARENT_SIZE)) is not None   # the parent's size is refused
