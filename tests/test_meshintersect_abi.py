"""CPU: the intersection kernels' place in the build, their two entry points and three constants, and the launchers'
host-side checks.  The feature adds no struct, no field and no version step: NudfPointCloud is read as include/nudf.h says."""
import ctypes as C
import math
import os
import re

import pytest

COUNT_BUFFERS = ("verts", "faces", "cell_start", "cell_count", "hash_key", "hash_row", "md_cell_face", "md_ref_n")
EMIT_BUFFERS = ("md_ref_off", "md_ref_key", "md_ref_face", "state")
ENTRIES = ("count", "emit")
POINT_CLOUD_BYTES = 472            # sizeof(NudfPointCloud) of the parent commit


def _desc(buffers=True, **kw):
    """a descriptor both entry points would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, n_query=4, cell=0.5, md_n_refs=12, n_cells=3, hash_cap=8, md_mode=0, cap=5)
    if buffers:
        args.update({b: 4096 for b in COUNT_BUFFERS + EMIT_BUFFERS})
    grid = kw.pop("grid", (3, 3, 3))
    args.update(kw)
    d = _lib.PointCloud(**args)
    d.grid[:] = grid
    return d


def _refused(lib, entry, d, word):
    assert getattr(lib, "nudf_pc_isect_" + entry)(C.byref(d), None) != 0, (entry, word)
    err = lib.nudf_last_error()
    assert b"nudf_pc_isect_" + entry.encode() in err and word in err, (entry, word, err)


def test_build_lists_the_source_symbols_and_constants():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshintersect.hip" in build.SOURCES
    assert build.KERNEL_SOURCES["meshintersect"] == ["csrc/meshintersect.hip", *build._CELL_INDEX, *build._MESH_COMMON]
    digest = build.source_digest("meshintersect")
    assert len(digest) == 16 and int(digest, 16) >= 0 and digest != build.source_digest("meshray")
    header = open(os.path.join(build.INCLUDE, "nudf.h")).read()
    for e in ENTRIES:
        name = "nudf_pc_isect_" + e
        assert name in _lib.SIGNATURES and name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert _lib.SIGNATURES[name][1][0] is C.POINTER(_lib.PointCloud)
        assert re.search(r"^int %s\(const NudfPointCloud\* args, void\* stream\);" % name, header, re.M)
    assert _lib.ISECT == dict(CROSSING=1, COPLANAR=2, UNCERTAIN=3)
    for k, v in _lib.ISECT.items():
        assert re.search(r"^#define NUDF_ISECT_%s %d\b" % (k, v), header, re.M), k
    src = open(os.path.join(build.CSRC, "meshintersect.hip")).read()
    code = [l for l in src.splitlines() if l.strip() and not l.startswith("//")]
    assert code[0] == "#pragma clang fp contract(off)"
    assert '#include "cell_index.h"' in code and '#include "mesh_launch.h"' in code
    assert "atomic" not in src.split("#pragma", 1)[1].lower()
    import meshintersect_ref as ref
    from neuraludf_amd import evaluation
    assert (ref.CROSSING, ref.COPLANAR, ref.UNCERTAIN) == tuple(_lib.ISECT[k] for k in ("CROSSING", "COPLANAR", "UNCERTAIN"))
    assert ref.MESH_CELL_FACTOR == evaluation.MESH_CELL_FACTOR
    assert evaluation.ISECT_KINDS == {k.lower(): v for k, v in _lib.ISECT.items()}


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
        _refused(lib, entry, _desc(**bad), b"cell")
    for bad in (dict(grid=(3, 0, 3)), dict(grid=(3, 3, (1 << 21) + 1)), dict(grid=(-1, 3, 3))):
        _refused(lib, entry, _desc(**bad), b"grid")
    for bad in (6, 4, 0):
        _refused(lib, entry, _desc(hash_cap=bad), b"hash_cap")
    _refused(lib, entry, _desc(n_cells=0), b"hash_cap")
    for n in ("n_query", "n_faces", "n_verts"):
        _refused(lib, entry, _desc(**{n: 1 << 31}), b"2^31")
    for bad in (2, -1, 17):
        _refused(lib, entry, _desc(md_mode=bad), b"mode")
    _refused(lib, entry, _desc(n_query=3), b"n_query == n_faces")
    _refused(lib, entry, _desc(cap=-1), b"cap")
    _refused(lib, entry, _desc(md_n_refs=0), b"no faces")
    _refused(lib, entry, _desc(buffers=False), b"NULL")
    for b in COUNT_BUFFERS:
        _refused(lib, entry, _desc(**{b: None}), b"NULL")
    _refused(lib, entry, _desc(md_mode=1, n_query=7), b"NULL")                 # two meshes: the corner coordinates
    # the largest grid is accepted as far as the host checks go: the refusal that is left is the missing buffers
    _refused(lib, entry, _desc(buffers=False, grid=(1 << 21, 1, 1 << 21)), b"NULL")


def test_emit_refuses_missing_output_buffers():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for b in EMIT_BUFFERS:
        _refused(lib, "emit", _desc(**{b: None}), b"NULL")


@pytest.mark.parametrize("entry", ENTRIES)
def test_launchers_accept_empty_descriptors(entry):
    from neuraludf_amd import _lib
    fn = getattr(_lib.lib(), "nudf_pc_isect_" + entry)
    assert fn(C.byref(_lib.PointCloud()), None) == 0
    # nothing to do, whatever the other fields say
    assert fn(C.byref(_desc(n_query=0, md_mode=9, cell=-1.0, buffers=False)), None) == 0
    if entry == "emit":                                    # no pair was accepted: nothing to write
        assert fn(C.byref(_desc(cap=0, md_mode=9, cell=-1.0, buffers=False)), None) == 0
