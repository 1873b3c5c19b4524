"""CPU: the texture kernels' place in the build and the launchers' host-side checks.  (The ctypes mirror of NudfMeshRaster
with its tx_ fields, its size in the library, the library version and the exports: tests/test_abi.py.)"""
import ctypes as C

ENTRIES = ("bake", "shade")


def test_build_lists_the_sources():
    from neuraludf_amd import build
    build.build()
    assert "meshtexture.hip" in build.SOURCES
    assert {"csrc/meshtexture.hip", "csrc/meshraster_pixel.h"} <= set(build.KERNEL_SOURCES["meshtexture"])
    assert len(build.source_digest("meshtexture")) == 16
    assert build.source_digest("meshtexture") != build.source_digest("meshraster")


def _desc(**fields):
    """a descriptor with one class of one cell of side 8 in an 8 x 8 atlas; pointers are fake and never dereferenced: every
    case below is refused or empty before a launch"""
    from neuraludf_amd import _lib
    d = _lib.MeshRaster(n_faces=2, n_verts=4, n_views=1, H=3, W=5, tx_W=8, tx_H=8, tx_n_cells=1, tx_n_classes=1)
    d.tx_class_k[0], d.tx_class_off[1], d.tx_class_cell[1] = 3, 64, 1
    for name, value in fields.items():
        if isinstance(value, tuple):
            getattr(d, name)[value[0]] = value[1]
        else:
            setattr(d, name, value)
    return d


def test_launchers_refuse_bad_descriptors_without_a_gpu():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for bad, word in ((dict(n_faces=1 << 31), b"2^31"), (dict(n_verts=-1), b"n_verts"), (dict(n_views=-1), b"n_views"),
                      (dict(H=-1), b"H"), (dict(H=1 << 16, W=1 << 15), b"H * W"),
                      (dict(n_views=1 << 10, H=1 << 15, W=1 << 15), b"2^38"), (dict(tx_W=-1), b"tx_W"),
                      (dict(tx_W=1 << 16, tx_H=1 << 15), b"tx_W * tx_H"), (dict(tx_n_cells=-1), b"tx_n_cells")):
        for e in ENTRIES:
            assert getattr(lib, "nudf_meshtexture_" + e)(C.byref(_desc(**bad)), None) != 0, (bad, e)
            msg = lib.nudf_last_error()
            assert b"nudf_meshtexture_" + e.encode() in msg and word in msg, (bad, e, msg)
    for bad, word in ((dict(tx_n_classes=11), b"tx_n_classes"), (dict(tx_n_classes=-1), b"tx_n_classes"),
                      (dict(tx_class_k=(0, 2)), b"tx_class_k"), (dict(tx_class_k=(0, 13)), b"tx_class_k"),
                      (dict(tx_class_off=(1, -64)), b"ascend"), (dict(tx_class_off=(0, 64)), b"start at 0"),
                      (dict(tx_class_cell=(1, -1)), b"ascend")):
        assert lib.nudf_meshtexture_bake(C.byref(_desc(**bad)), None) != 0, bad
        assert word in lib.nudf_last_error(), (bad, lib.nudf_last_error())
    # NULL buffers: the outputs first, then what an owned texel reads, then what a view reads
    assert lib.nudf_meshtexture_bake(C.byref(_desc()), None) != 0 and b"tx_colors" in lib.nudf_last_error()
    out = dict(tx_colors=4096, tx_n_seen=4096)
    assert lib.nudf_meshtexture_bake(C.byref(_desc(**out)), None) != 0 and b"tx_uv" in lib.nudf_last_error()
    mesh = dict(out, tx_uv=4096, tx_cell_face=4096, faces=4096, pos=4096)
    assert lib.nudf_meshtexture_bake(C.byref(_desc(**mesh)), None) != 0 and b"proj" in lib.nudf_last_error()
    views = dict(mesh, proj=4096, depth=4096, images=4096)
    assert lib.nudf_meshtexture_bake(C.byref(_desc(**views, normals=4096)), None) != 0
    assert b"cam_pos" in lib.nudf_last_error()
    for power in (float("nan"), float("inf")):
        assert lib.nudf_meshtexture_bake(C.byref(_desc(**views, normals=4096, cam_pos=4096, power=power)), None) != 0
        assert b"power" in lib.nudf_last_error()
    assert lib.nudf_meshtexture_bake(C.byref(_desc(**views, H=0)), None) != 0 and b"H and W" in lib.nudf_last_error()
    assert lib.nudf_meshtexture_shade(C.byref(_desc()), None) != 0 and b"face" in lib.nudf_last_error()
    shade = dict(face=4096, bary=4096, tx_out=4096, tx_colors=4096)
    assert lib.nudf_meshtexture_shade(C.byref(_desc(**shade)), None) != 0 and b"tx_uv" in lib.nudf_last_error()
    assert lib.nudf_meshtexture_shade(C.byref(_desc(**shade, tx_uv=4096, tx_W=0)), None) != 0
    assert b"tx_W and tx_H" in lib.nudf_last_error()


def test_empty_descriptors_return_zero_without_a_gpu():
    from neuraludf_amd import _lib
    lib = _lib.lib()
    for e in ENTRIES:
        assert getattr(lib, "nudf_meshtexture_" + e)(C.byref(_lib.MeshRaster()), None) == 0, e
    assert lib.nudf_meshtexture_bake(C.byref(_desc(tx_W=0, tx_H=0)), None) == 0          # an atlas of no texels
    assert lib.nudf_meshtexture_bake(C.byref(_desc(tx_H=0)), None) == 0
    for none in (dict(n_views=0), dict(H=0), dict(W=0)):                                   # no pixels to shade
        assert lib.nudf_meshtexture_shade(C.byref(_desc(**none)), None) == 0, none
