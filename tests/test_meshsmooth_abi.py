"""CPU: the smoothing kernels' place in the build, the launchers' host-side checks, and the way NudfMeshOrient grew: at its
end only, under the same ABI version.  (The ctypes mirror against the header, its size in the library and the exports:
tests/test_abi.py.)"""
import ctypes as C
import math
import os
import re

ENTRIES = ("laplace", "frames", "normals", "update")
ORIENT_FIELDS = ["faces", "me_a", "me_b", "word", "changed", "nonorient", "comp_off", "comp_face", "comp_sum", "pos",
                 "corner_off", "corner", "normals", "origin", "n_faces", "n_verts", "n_medges", "n_comps"]
SMOOTH_FIELDS = ["sm_nbr_off", "sm_nbr", "sm_fixed", "sm_pos_out", "sm_fnormal", "sm_fnormal_out", "sm_farea", "sm_fcentre",
                 "sm_n_nbr", "sm_step", "sm_inv2sc", "sm_inv2ss", "sm_weights", "sm_pad_"]
BUFFERS = ("faces", "pos", "corner_off", "corner", "sm_nbr_off", "sm_nbr", "sm_pos_out", "sm_fnormal", "sm_fnormal_out",
           "sm_farea", "sm_fcentre")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nudf.h")


def _desc(buffers=True, **kw):
    """a descriptor every entry point would launch (fake non-NULL addresses: a refused call never dereferences them)"""
    from neuraludf_amd import _lib
    args = dict(n_faces=4, n_verts=8, sm_n_nbr=12, sm_step=0.5, sm_inv2sc=2.0, sm_inv2ss=4.0, sm_weights=0)
    if buffers:
        args.update({b: 4096 for b in BUFFERS})
    args.update(kw)
    return _lib.MeshOrient(**args)


def _call(lib, entry, d):
    return getattr(lib, "nudf_meshsmooth_" + entry)(C.byref(d), None)


def _refused(lib, entry, d, word):
    assert _call(lib, entry, d) != 0, (entry, word)
    err = lib.nudf_last_error()
    assert b"nudf_meshsmooth_" + entry.encode() in err and word in err, (entry, word, err)


def test_build_lists_the_source():
    from neuraludf_amd import build, _lib
    build.build()
    assert "meshsmooth.hip" in build.SOURCES
    assert "csrc/meshsmooth.hip" in build.KERNEL_SOURCES["meshsmooth"]
    assert len(build.source_digest("meshsmooth")) == 16
    for e in ENTRIES:
        assert "nudf_meshsmooth_" + e in _lib.SIGNATURES and hasattr(_lib.lib(), "nudf_meshsmooth_" + e)
        assert _lib.SIGNATURES["nudf_meshsmooth_" + e][1][0] is C.POINTER(_lib.MeshOrient)


def test_launchers_refuse_without_a_gpu():
    """the checks are host code: no kernel is launched for a refused descriptor"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        _refused(lib, e, _desc(n_verts=1 << 31), b"2^31")
        for bad in (dict(n_faces=-1), dict(n_verts=-1), dict(n_faces=1 << 36), dict(sm_n_nbr=-1)):
            _refused(lib, e, _desc(**bad), b"bad sizes")
        _refused(lib, e, _desc(buffers=False), b"NULL")
    for bad in (math.nan, math.inf, -math.inf):
        _refused(lib, "laplace", _desc(sm_step=bad), b"sm_step")
    for bad in (2, -1, 7):
        _refused(lib, "laplace", _desc(sm_weights=bad), b"sm_weights")
    for b in ("pos", "sm_pos_out", "sm_nbr_off", "sm_nbr"):
        _refused(lib, "laplace", _desc(**{b: None}), b"NULL")
    for b in ("pos", "sm_pos_out", "corner_off", "corner", "faces"):
        _refused(lib, "laplace", _desc(sm_weights=1, **{b: None}), b"NULL")
    for b in ("faces", "pos", "sm_fnormal_out", "sm_farea", "sm_fcentre"):
        _refused(lib, "frames", _desc(**{b: None}), b"NULL")
    for field in ("sm_inv2sc", "sm_inv2ss"):
        for bad in (0.0, -1.0, math.nan, math.inf):
            _refused(lib, "normals", _desc(**{field: bad}), b"sigma")
    for b in ("faces", "corner_off", "corner", "sm_fnormal", "sm_fnormal_out", "sm_farea", "sm_fcentre"):
        _refused(lib, "normals", _desc(**{b: None}), b"NULL")
    for b in ("pos", "sm_pos_out", "corner_off", "corner", "faces", "sm_fnormal"):
        _refused(lib, "update", _desc(**{b: None}), b"NULL")


def test_launchers_accept_empty_descriptors():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        assert _call(lib, e, _lib.MeshOrient()) == 0, e
    # nothing to do for this entry point, whatever the other fields say
    for e in ("laplace", "update"):
        assert _call(lib, e, _desc(buffers=False, n_verts=0, sm_weights=9, sm_step=math.nan)) == 0, e
    for e in ("frames", "normals"):
        assert _call(lib, e, _desc(buffers=False, n_faces=0, sm_inv2sc=-1.0)) == 0, e


def test_mesh_orient_grew_at_its_end_only():
    """the orientation fields keep their places, n_comps is followed directly by the first sm_ field, and nothing but sm_
    fields follows"""
    from neuraludf_amd import _lib
    M = _lib.MeshOrient
    names = [f[0] for f in M._fields_]
    assert names == ORIENT_FIELDS + SMOOTH_FIELDS
    offsets = [getattr(M, n).offset for n in ORIENT_FIELDS]
    assert offsets == [8 * i for i in range(13)] + [104, 128, 136, 144, 152]          # 13 pointers, double[3], four counts
    assert M.sm_nbr_off.offset == M.n_comps.offset + 8 == 160
    assert all(n.startswith("sm_") for n in names[names.index("n_comps") + 1:])
    assert M.sm_pad_.offset + 4 == C.sizeof(M) == 264      # eight pointers, a count, three doubles, two words


def test_version_and_struct_count_are_unchanged():
    from neuraludf_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define NUDF_ABI_VERSION 111$", text, re.M)
    assert _lib.ABI_VERSION == 111 == _lib.lib().nudf_version()
    assert len(_lib.MIRRORS) == 31
    version, table = _lib._abi_report(_lib.lib())
    assert version == 111 and len(table) == 31 and table["NudfMeshOrient"] == C.sizeof(_lib.MeshOrient)
    assert _lib._abi_mismatch(version, dict(table, NudfMeshOrient=160)) is not None    # the parent's size is refused
