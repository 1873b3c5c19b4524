"""CPU: the subdivision kernels' place in the build, the launchers' host-side checks, and the way NudfMeshTopo grew: at its
end only, under the same ABI version.  (The ctypes mirror against the header, its size in the library and the exports:
tests/test_abi.py.)"""
import ctypes as C
import math
import os
import re

ENTRIES = ("mark", "odd", "even", "count", "emit")
# offsets of the simplification's fields before the subdivision's were appended
PARENT_OFFSETS = dict(sp_key=232, sp_cluster_key=240, sp_vcluster=248, sp_member_off=256, sp_member=264, sp_corner_off=272,
                      sp_corner=280, sp_attr=288, sp_rep=296, sp_accepted=304, sp_quadric=312, sp_attr_out=320,
                      sp_faces=328, sp_triple=336, sp_degenerate=344, n_clusters=352, sp_grid=360, sp_origin=384,
                      sp_cell=408, sp_lambda=416, sp_boundary_weight=424, sp_attr_width=432, sp_placement=436)
PARENT_SIZE = 440
BUFFERS = ("faces", "edges", "he_edge", "he_id", "edge_start", "nbr_off", "nbr", "pos", "sp_attr", "sp_sd_mark",
           "sp_sd_edge_vertex", "sp_sd_marked", "sp_sd_ring_off", "sp_sd_ring", "sp_sd_vclass", "sp_sd_pos_out",
           "sp_sd_attr_out", "sp_sd_fcount", "sp_sd_foff", "sp_sd_faces_out", "sp_sd_parent")
READS = dict(mark=("edges", "sp_sd_mark", "pos"),
             odd=("sp_sd_marked", "edges", "pos", "sp_sd_pos_out", "sp_attr", "sp_sd_attr_out", "faces", "he_id", "edge_start"),
             even=("pos", "sp_sd_pos_out", "sp_attr", "sp_sd_attr_out", "sp_sd_vclass", "sp_sd_ring_off", "sp_sd_ring",
                   "nbr_off", "nbr"),
             count=("faces", "he_edge", "sp_sd_edge_vertex", "sp_sd_fcount"),
             emit=("faces", "he_edge", "sp_sd_edge_vertex", "sp_sd_foff", "sp_sd_faces_out", "sp_sd_parent", "sp_sd_pos_out"))
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nudf.h")


def _desc(buffers=True, **kw):
    """a descriptor every entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, n_edges=9, sp_attr_width=3, sp_sd_n_ring=18, sp_sd_n_border=8, sp_sd_n_marked=5,
                sp_sd_n_out=12, sp_sd_max_edge=0.5, sp_sd_scheme=1, sp_sd_mark_all=0)
    if buffers:
        args.update({b: 4096 for b in BUFFERS})
    args.update(kw)
    return _lib.MeshTopo(**args)


def _call(lib, entry, d):
    return getattr(lib, "nudf_meshsubdiv_" + entry)(C.byref(d), None)


def _refused(lib, entry, d, word):
    assert _call(lib, entry, d) != 0, (entry, word)
    err = lib.nudf_last_error()
    assert b"nudf_meshsubdiv_" + entry.encode() in err and word in err, (entry, word, err)


def test_build_lists_the_source():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshsubdiv.hip" in build.SOURCES
    assert "csrc/meshsubdiv.hip" in build.KERNEL_SOURCES["meshsubdiv"]
    assert len(build.source_digest("meshsubdiv")) == 16
    for e in ENTRIES:
        assert "nudf_meshsubdiv_" + e in _lib.SIGNATURES and "nudf_meshsubdiv_" + e in _lib.SYMBOLS
        assert hasattr(_lib.lib(), "nudf_meshsubdiv_" + e)
        assert _lib.SIGNATURES["nudf_meshsubdiv_" + e][1][0] is C.POINTER(_lib.MeshTopo)
    assert re.search(r"^int nudf_meshsubdiv_emit\(const NudfMeshTopo\* args, void\* stream\);", open(HEADER).read(), re.M)


def test_launchers_refuse_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        for bad, word in ((dict(n_faces=-1), b"n_faces"), (dict(n_faces=1 << 31), b"n_faces"), (dict(n_verts=-1), b"n_verts"),
                          (dict(n_verts=1 << 31), b"2^31"), (dict(n_edges=-1), b"n_edges"), (dict(n_edges=13), b"n_edges"),
                          (dict(sp_sd_n_marked=-1), b"sp_sd_n_marked"), (dict(sp_sd_n_marked=10), b"sp_sd_n_marked"),
                          (dict(sp_sd_n_out=-1), b"sp_sd_n_out"), (dict(sp_sd_n_out=17), b"sp_sd_n_out"),
                          (dict(sp_sd_n_ring=-1), b"sp_sd_n_ring"), (dict(sp_sd_n_border=-1), b"sp_sd_n_border"),
                          (dict(sp_attr_width=-1), b"sp_attr_width")):
            _refused(lib, e, _desc(**bad), word)
        # old and new vertices together must stay below 2^31
        big = dict(n_verts=(1 << 31) - 3, n_faces=1 << 30, n_edges=1 << 30, sp_sd_n_marked=3)
        _refused(lib, e, _desc(**big), b"n_verts + sp_sd_n_marked")
        _refused(lib, e, _desc(buffers=False), b"NULL")
        for b in READS[e]:
            _refused(lib, e, _desc(**{b: None}), b"NULL")
            assert b.encode() in lib.nudf_last_error(), (e, b)
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        _refused(lib, "mark", _desc(sp_sd_max_edge=bad), b"sp_sd_max_edge")
    for e in ("odd", "even"):
        for bad in (2, -1, 7):
            _refused(lib, e, _desc(sp_sd_scheme=bad), b"sp_sd_scheme")


def test_launchers_accept_what_they_do_not_read():
    """refusals are about the fields an entry point uses: a descriptor passes the host checks only as far as the launch,
    so these are checked through the order of the refusals -- the next one in line is reported"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    # with sp_sd_mark_all the length bound and the positions are not read: the refusal is about the NULL that remains
    _refused(lib, "mark", _desc(sp_sd_mark_all=1, sp_sd_max_edge=math.nan, pos=None, sp_sd_mark=None), b"NULL")
    # midpoint reads no adjacency: the refusal is about the buffer taken away besides
    _refused(lib, "even", _desc(sp_sd_scheme=0, sp_sd_vclass=None, sp_sd_ring_off=None, nbr_off=None, pos=None), b"NULL pos")
    _refused(lib, "odd", _desc(sp_sd_scheme=0, faces=None, he_id=None, edge_start=None, pos=None), b"NULL sp_sd_marked, edges, pos")
    # without attributes their buffers are not read
    _refused(lib, "odd", _desc(sp_attr_width=0, sp_attr=None, sp_sd_attr_out=None, he_id=None), b"NULL faces, he_id")


def test_launchers_accept_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        assert _call(lib, e, _lib.MeshTopo()) == 0, e
    # nothing to do for this entry point, whatever the other fields say
    empty = dict(buffers=False, sp_sd_max_edge=math.nan, sp_sd_scheme=9)
    assert _call(lib, "mark", _desc(n_edges=0, sp_sd_n_marked=0, **empty)) == 0
    assert _call(lib, "odd", _desc(sp_sd_n_marked=0, **empty)) == 0
    assert _call(lib, "even", _desc(n_verts=0, **empty)) == 0
    for e in ("count", "emit"):
        assert _call(lib, e, _desc(n_faces=0, n_edges=0, sp_sd_n_marked=0, sp_sd_n_out=0, **empty)) == 0, e


def test_mesh_topo_grew_at_its_end_only():
    """the simplification's fields keep the parent's offsets, sp_placement is followed directly by the first sp_sd_ field,
    and nothing but sp_sd_ fields follows"""
    from neuraludf_amd import _lib
    M = _lib.MeshTopo
    names = [f[0] for f in M._fields_]
    first, last = names.index("sp_key"), names.index("sp_placement")
    assert names[first:last + 1] == list(PARENT_OFFSETS)
    assert {n: getattr(M, n).offset for n in PARENT_OFFSETS} == PARENT_OFFSETS
    tail = names[last + 1:]
    assert tail and all(n.startswith("sp_sd_") for n in tail)
    assert getattr(M, tail[0]).offset == M.sp_placement.offset + 4 == PARENT_SIZE
    assert C.sizeof(M) > PARENT_SIZE and C.sizeof(M) % 8 == 0
    text = open(HEADER).read()
    struct = text[text.index("typedef struct NudfMeshTopo {"):text.index("} NudfMeshTopo;")]
    declared = re.findall(r"^\s+(?:const )?\w+\*? (\w+)(?:\[\d+\])?;", struct, re.M)
    assert declared == names


def test_version_and_struct_count_are_unchanged():
    from neuraludf_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define NUDF_ABI_VERSION 111$", text, re.M)
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()
    assert len(_lib.MIRRORS) == 31
    version, table = _lib._abi_report(_lib.lib())
    assert version == 111 and len(table) == 31 and table["NudfMeshTopo"] == C.sizeof(_lib.MeshTopo)
    assert _lib._abi_mismatch(version, dict(table, NudfMeshTopo=PARENT_SIZE)) is not None   # the parent's size is refused
