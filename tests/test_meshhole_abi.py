"""CPU: the hole-closing kernels' place in the build, the launchers' host-side checks, and the way NudfMeshTopo grew: after
the subdivision's fields only, under the same ABI version.  (The ctypes mirror against the header, its size in the library
and the exports: tests/test_abi.py; the sp_sd_ prefix of the tail: tests/test_meshsubdiv_abi.py.)"""
import ctypes as C
import math
import os
import re

ENTRIES = ("link", "rank", "count", "triangulate")
BUFFERS = ("faces", "edges", "he_edge", "edge_key", "pos", "new_count", "new_off", "new_faces", "sp_sd_hf_bedge",
           "sp_sd_hf_brank", "sp_sd_hf_link", "sp_sd_hf_rank_in", "sp_sd_hf_loop_off", "sp_sd_hf_loop_vertex",
           "sp_sd_hf_loop_edge", "sp_sd_hf_closed", "sp_sd_hf_perimeter", "sp_sd_hf_status")
READS = dict(link=("faces", "edges", "he_edge", "sp_sd_hf_bedge", "sp_sd_hf_brank", "sp_sd_hf_link"),
             rank=("sp_sd_hf_rank_in", "sp_sd_hf_rank_out"),
             count=("edges", "pos", "sp_sd_hf_loop_off", "sp_sd_hf_loop_vertex", "sp_sd_hf_loop_edge", "sp_sd_hf_closed",
                    "sp_sd_hf_perimeter", "sp_sd_hf_status", "new_count"),
             triangulate=("faces", "edges", "he_edge", "edge_key", "pos", "sp_sd_hf_loop_off", "sp_sd_hf_loop_vertex",
                          "sp_sd_hf_loop_edge", "sp_sd_hf_status", "new_off", "new_faces"))
# the subdivision's last field and the size of the struct before the hole closing's fields were appended
PARENT_LAST, PARENT_SIZE = "sp_sd_mark_all", 584
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nudf.h")


def _desc(buffers=True, **kw):
    """a descriptor every entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=8, n_verts=9, n_edges=16, sp_sd_hf_n_border=8, sp_sd_hf_n_loops=2, sp_sd_hf_n_items=8, n_new=4,
                max_loop=32, sp_sd_hf_max_perimeter=math.inf, sp_sd_hf_round=1)
    if buffers:
        args.update({b: 4096 for b in BUFFERS}, sp_sd_hf_rank_out=8192)
    args.update(kw)
    return _lib.MeshTopo(**args)


def _call(lib, entry, d):
    return getattr(lib, "nudf_meshhole_" + entry)(C.byref(d), None)


def _refused(lib, entry, d, word):
    assert _call(lib, entry, d) != 0, (entry, word)
    err = lib.nudf_last_error()
    assert b"nudf_meshhole_" + entry.encode() in err and word in err, (entry, word, err)


def test_build_lists_the_source():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshhole.hip" in build.SOURCES
    assert build.KERNEL_SOURCES["meshhole"] == ["csrc/meshhole.hip", *build._MESH_COMMON]
    assert len(build.source_digest("meshhole")) == 16
    text = open(HEADER).read()
    for e in ENTRIES:
        assert "nudf_meshhole_" + e in _lib.SIGNATURES and "nudf_meshhole_" + e in _lib.SYMBOLS
        assert hasattr(_lib.lib(), "nudf_meshhole_" + e)
        assert _lib.SIGNATURES["nudf_meshhole_" + e][1][0] is C.POINTER(_lib.MeshTopo)
        assert re.search(r"^int nudf_meshhole_%s\(const NudfMeshTopo\* args, void\* stream\);" % e, text, re.M)
    src = open(os.path.join(os.path.dirname(build.__file__), "csrc", "meshhole.hip")).read()
    code = [ln for ln in src.splitlines() if ln.strip() and not ln.lstrip().startswith("//")]
    assert code[0] == "#pragma clang fp contract(off)"


def test_constants_equal_the_header():
    from neuraludf_amd import _lib, meshclean
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    codes = {k: int(v) for k, v in re.findall(r"\bNUDF_HOLE_(\w+) = (\d+)", text)}
    assert codes == _lib.HOLE and len(set(codes.values())) == 7
    assert int(re.search(r"^#define NUDF_HOLE_MAX_EDGES (\d+)", text, re.M).group(1)) == _lib.HOLE_MAX_EDGES == 64
    assert int(re.search(r"^#define NUDF_HOLE_FAN_CAP (\d+)", text, re.M).group(1)) == _lib.HOLE_FAN_CAP
    assert meshclean.MAX_HOLE_EDGES == 64
    for k, v in _lib.HOLE.items():
        assert getattr(meshclean, "HOLE_" + k) == v
    import meshhole_ref as ref
    assert [ref.FILLED, ref.OPEN_CHAIN, ref.TOO_MANY_EDGES, ref.PERIMETER, ref.NONFINITE, ref.DUPLICATE,
            ref.REPEATED_VERTEX] == [_lib.HOLE[k] for k in ("FILLED", "OPEN_CHAIN", "TOO_MANY_EDGES", "PERIMETER",
                                                            "NONFINITE", "DUPLICATE", "REPEATED_VERTEX")]
    assert ref.MAX_HOLE_EDGES == _lib.HOLE_MAX_EDGES and ref.FAN_CAP == _lib.HOLE_FAN_CAP


def test_launchers_refuse_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        for bad, word in ((dict(n_faces=-1), b"n_faces"), (dict(n_faces=1 << 31), b"n_faces"), (dict(n_verts=-1), b"n_verts"),
                          (dict(n_verts=1 << 31), b"2^31"), (dict(n_edges=-1), b"n_edges"), (dict(n_edges=25), b"n_edges"),
                          (dict(sp_sd_hf_n_border=-1), b"sp_sd_hf_n_border"), (dict(sp_sd_hf_n_border=17), b"sp_sd_hf_n_border"),
                          (dict(sp_sd_hf_n_loops=-1), b"sp_sd_hf_n_loops"), (dict(sp_sd_hf_n_loops=9), b"sp_sd_hf_n_loops"),
                          (dict(sp_sd_hf_n_items=-1), b"sp_sd_hf_n_items"), (dict(sp_sd_hf_n_items=9), b"sp_sd_hf_n_items"),
                          (dict(n_new=-1), b"n_new"), (dict(n_new=9), b"n_new")):
            _refused(lib, e, _desc(**bad), word)
        _refused(lib, e, _desc(buffers=False), b"NULL")
        for b in READS[e]:
            _refused(lib, e, _desc(**{b: None}), b"NULL")
            assert b.encode() in lib.nudf_last_error(), (e, b)
    for e in ("count", "triangulate"):
        for bad in (2, 65, 0, -1):
            _refused(lib, e, _desc(max_loop=bad), b"max_loop")
        assert b"[3, 64]" in lib.nudf_last_error()
    for bad in (0.0, -1.0, math.nan, -math.inf):
        _refused(lib, "count", _desc(sp_sd_hf_max_perimeter=bad), b"sp_sd_hf_max_perimeter")
    for bad in (-1, 41):
        _refused(lib, "rank", _desc(sp_sd_hf_round=bad), b"sp_sd_hf_round")
    _refused(lib, "rank", _desc(sp_sd_hf_rank_out=4096), b"must differ")


def test_launchers_accept_what_they_do_not_read():
    """refusals are about the fields an entry point uses, checked through their order: the next one in line is reported"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    # link and rank read neither the longest loop nor the perimeter bound
    _refused(lib, "link", _desc(max_loop=99, sp_sd_hf_max_perimeter=-1.0, pos=None, faces=None), b"NULL faces")
    _refused(lib, "rank", _desc(max_loop=0, sp_sd_hf_max_perimeter=math.nan, faces=None, sp_sd_hf_rank_in=None), b"NULL sp_sd_hf_rank_in")
    # triangulate does not read the perimeter bound, the closed flags or the perimeters
    _refused(lib, "triangulate", _desc(sp_sd_hf_max_perimeter=0.0, sp_sd_hf_closed=None, sp_sd_hf_perimeter=None, pos=None),
             b"NULL faces, edges, he_edge, edge_key, pos")


def test_launchers_accept_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        assert _call(lib, e, _lib.MeshTopo()) == 0, e
    # nothing to do for this entry point, whatever the other fields say
    empty = dict(buffers=False, max_loop=0, sp_sd_hf_max_perimeter=math.nan)
    for e in ("link", "rank"):
        assert _call(lib, e, _desc(sp_sd_hf_n_border=0, sp_sd_hf_n_loops=0, sp_sd_hf_n_items=0, n_new=0, **empty)) == 0, e
    assert _call(lib, "count", _desc(sp_sd_hf_n_loops=0, **empty)) == 0
    assert _call(lib, "triangulate", _desc(sp_sd_hf_n_loops=0, **empty)) == 0
    assert _call(lib, "triangulate", _desc(n_new=0, **empty)) == 0


def test_mesh_topo_grew_after_the_subdivision_only():
    from neuraludf_amd import _lib
    M = _lib.MeshTopo
    names = [f[0] for f in M._fields_]
    tail = names[names.index(PARENT_LAST) + 1:]
    assert tail and all(n.startswith("sp_sd_hf_") for n in tail)
    assert not any(n.startswith("sp_sd_hf_") for n in names[:names.index(PARENT_LAST) + 1])
    assert getattr(M, tail[0]).offset == getattr(M, PARENT_LAST).offset + 4 == PARENT_SIZE
    assert C.sizeof(M) > PARENT_SIZE and C.sizeof(M) % 8 == 0


def test_version_and_struct_count_are_unchanged():
    from neuraludf_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define NUDF_ABI_VERSION 111$", text, re.M)
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()
    assert len(_lib.MIRRORS) == 31
    version, table = _lib._abi_report(_lib.lib())
    assert table["NudfMeshTopo"] == C.sizeof(_lib.MeshTopo)
    assert _lib._abi_mismatch(version, dict(table, NudfMeshTopo=PARENT_SIZE)) is not None   # the parent's size is refused
