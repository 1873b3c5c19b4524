"""CPU: the winding-number kernels' place in the build, their three entry points and the launchers' host-side checks.  The
feature adds no struct, no field and no version step: NudfPointCloud is read as include/nudf.h says."""
import ctypes as C
import math
import os
import re

import pytest

ENTRIES = ("nudf_pc_wn_faces", "nudf_pc_wn_nodes", "nudf_pc_winding")
BUFFERS = {
    "nudf_pc_wn_faces": ("verts", "faces", "keys"),
    "nudf_pc_wn_nodes": ("verts", "faces", "md_cell_face", "rank", "cell_start", "cell_count", "query_idx", "out", "md_point"),
    "nudf_pc_winding": ("verts", "faces", "md_cell_face", "pts", "rank", "cell_start", "cell_count", "query", "dist"),
}
POINT_CLOUD_BYTES = 472            # sizeof(NudfPointCloud) of the parent commit


def _desc(entry, buffers=True, **kw):
    """a descriptor the entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, n_query=4, cell=0.5, md_n_refs=4, n=3, md_mode=0, r2=4.0)
    if buffers:
        args.update({b: 4096 for b in BUFFERS[entry]})
    grid = kw.pop("grid", (3, 3, 3))
    origin = kw.pop("origin", (0.0, 0.0, 0.0))
    args.update(kw)
    d = _lib.PointCloud(**args)
    d.grid[:], d.origin[:] = grid, origin
    return d


def _refused(lib, entry, d, word):
    assert getattr(lib, entry)(C.byref(d), None) != 0, (entry, word)
    err = lib.nudf_last_error()
    assert entry.encode() + b":" in err and word in err, (entry, word, err)


def test_build_lists_the_source_symbols_and_header_text():
    from neuraludf_amd import build, _lib, evaluation
    build.build()
    assert "meshwinding.hip" in build.SOURCES
    assert build.KERNEL_SOURCES["meshwinding"] == ["csrc/meshwinding.hip", *build._CELL_INDEX, *build._MESH_COMMON]
    digest = build.source_digest("meshwinding")
    assert len(digest) == 16 and int(digest, 16) >= 0 and digest != build.source_digest("meshintersect")
    header = open(os.path.join(build.INCLUDE, "nudf.h")).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert _lib.SIGNATURES[name][0] is C.c_int and _lib.SIGNATURES[name][1] == [C.POINTER(_lib.PointCloud), C.c_void_p]
        assert re.search(r"^int %s\(const NudfPointCloud\* args, void\* stream\);" % name, header, re.M)
    # the header says which fields each entry point reads and with what meaning
    block = header[header.index("Generalised winding numbers"):header.index("int nudf_pc_wn_faces")]
    for word in ("wn_faces", "wn_nodes", "winding", "keys[t]", "md_cell_face", "rank[i] = skip[i]", "cell_start / cell_count",
                 "query_idx", "out[40 i", "md_point[32 i", "pts [n, 32]", "r2 = beta * beta", "dist[", "md_count[", "idx[",
                 "NO new struct, field or version step", "Host-side refusals"):
        assert word in block, word
    src = open(os.path.join(build.CSRC, "meshwinding.hip")).read()
    code = [l for l in src.splitlines() if l.strip() and not l.startswith("//")]
    assert code[0] == "#pragma clang fp contract(off)"
    assert '#include "cell_index.h"' in code and '#include "mesh_launch.h"' in code
    body = src.split("#pragma", 1)[1].lower()
    assert "atomic" not in body and "asm" not in body and "__shared__" not in body
    assert "__builtin_amdgcn_readfirstlane" in src
    import meshwinding_ref as ref
    assert ref.WINDING_LEAF_FACTOR == evaluation.WINDING_LEAF_FACTOR and ref.AXIS_CELLS == evaluation.AXIS_CELLS
    assert (evaluation.WINDING_RAW, evaluation.WINDING_REC) == tuple(
        int(re.search(r"^#define %s (\d+)" % k, src, re.M).group(1)) for k in ("WN_RAW", "WN_REC"))
    assert evaluation.WINDING_REC <= 32


def test_no_struct_no_field_no_version_step():
    from neuraludf_amd import _lib
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()
    version, table = _lib._abi_report(_lib.lib())
    assert len(table) == 31 == len(_lib.MIRRORS)
    assert table["NudfPointCloud"] == C.sizeof(_lib.PointCloud) == POINT_CLOUD_BYTES
    assert _lib.PointCloud._fields_[-1][0] == "md_count"


@pytest.mark.parametrize("entry", ENTRIES)
def test_launchers_refuse_without_a_gpu(entry):
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf)):
        _refused(lib, entry, _desc(entry, **bad), b"cell")
    for bad in (dict(grid=(3, 0, 3)), dict(grid=(3, 3, (1 << 21) + 1)), dict(grid=(-1, 3, 3))):
        _refused(lib, entry, _desc(entry, **bad), b"grid")
    for bad in ((math.nan, 0, 0), (0, math.inf, 0)):
        _refused(lib, entry, _desc(entry, origin=bad), b"origin")
    for n in ("n_query", "n_faces", "n_verts", "n", "md_n_refs"):
        _refused(lib, entry, _desc(entry, **{n: 1 << 31}), b"2^31")
    for n in ("n_faces", "n_verts", "n", "md_n_refs"):
        _refused(lib, entry, _desc(entry, **{n: -1}), b"2^31")
    _refused(lib, entry, _desc(entry, buffers=False), b"NULL")
    for b in BUFFERS[entry]:
        _refused(lib, entry, _desc(entry, **{b: None}), b"NULL")
    # the largest grid is accepted as far as the host checks go: the refusal that is left is the missing buffers
    _refused(lib, entry, _desc(entry, buffers=False, grid=(1 << 21, 1, 1 << 21)), b"NULL")


def test_faces_refuses_an_unknown_mode_and_a_face_count_that_differs():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad in (2, -1, 17):
        _refused(lib, "nudf_pc_wn_faces", _desc("nudf_pc_wn_faces", md_mode=bad), b"mode")
    _refused(lib, "nudf_pc_wn_faces", _desc("nudf_pc_wn_faces", n_query=3), b"n_query == n_faces")
    _refused(lib, "nudf_pc_wn_faces", _desc("nudf_pc_wn_faces", md_mode=1, n_query=7), b"NULL")       # point mode: query
    _refused(lib, "nudf_pc_wn_faces", _desc("nudf_pc_wn_faces", md_mode=1, n_query=7, query=4096, keys=None), b"NULL")


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_nodes_and_walk_refuse_an_empty_tree(entry):
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad in (dict(n=0), dict(md_n_refs=0), dict(n_faces=0)):
        _refused(lib, entry, _desc(entry, **bad), b"no nodes or no faces")


def test_walk_refuses_beta_below_one():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad in (0.99, 0.0, -4.0, math.nan):
        _refused(lib, "nudf_pc_winding", _desc("nudf_pc_winding", r2=bad), b"beta")
    # 1 and inf pass the check: what is left to refuse is the missing buffers
    for ok in (1.0, math.inf):
        _refused(lib, "nudf_pc_winding", _desc("nudf_pc_winding", r2=ok, buffers=False), b"NULL")


@pytest.mark.parametrize("entry", ENTRIES)
def test_launchers_accept_empty_descriptors(entry):
    from neuraludf_amd import _lib
    fn = getattr(_lib.lib(), entry)
    assert fn(C.byref(_lib.PointCloud()), None) == 0
    # nothing to do, whatever the other fields say
    assert fn(C.byref(_desc(entry, n_query=0, md_mode=9, cell=-1.0, r2=0.0, buffers=False)), None) == 0
