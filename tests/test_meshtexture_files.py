"""CPU: the OBJ / MTL / PNG triple of a textured mesh (neuraludf_amd/meshing.py write_obj, read_obj)."""
import numpy as np
import pytest


def _mesh():
    rng = np.random.default_rng(4)
    v = rng.standard_normal((6, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5]], dtype=np.int64)
    W, H = 16, 8
    ij = np.stack([rng.integers(0, W, (3, 3)), rng.integers(0, H, (3, 3))], -1)
    uv = ((ij + 0.5) / [W, H]).astype(np.float32)                # what extract_udf_mesh returns: exact in float32
    tex = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return v, f, uv, tex


def test_write_obj_read_obj_round_trip(tmp_path):
    from neuraludf_amd import meshing
    v, f, uv, tex = _mesh()
    meshing.write_obj(tmp_path / "a.obj", v, f, uv, tex)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.mtl", "a.obj", "a.png"]
    rv, rf, ruv, rtex = meshing.read_obj(tmp_path / "a.obj")
    assert rv.dtype == np.float64 and rf.dtype == np.int64 and ruv.shape == (3, 3, 2) and rtex.dtype == np.uint8
    assert np.array_equal(rv.astype(np.float32), v) and np.array_equal(rf, f)
    assert np.array_equal(ruv, uv.astype(np.float64)) and rtex.tobytes() == tex.tobytes()
    text = (tmp_path / "a.obj").read_text().splitlines()
    assert text[0] == "mtllib a.mtl" and sum(ln.startswith("vt ") for ln in text) == 9
    assert text[-1] == "f 4/7 5/8 6/9" and "map_Kd a.png" in (tmp_path / "a.mtl").read_text()
    # float64 vertices and float textures: the digits float64 needs, colours rounded as write_ply rounds them
    v64 = np.random.default_rng(5).standard_normal((6, 3))
    texf = np.array([[[0.0, 0.5, 1.0], [0.2, 1.5, -1.0]]])
    meshing.write_obj(tmp_path / "b.obj", v64, f, uv.astype(np.float64), texf)
    rv, _, ruv, rtex = meshing.read_obj(tmp_path / "b.obj")
    assert np.array_equal(rv, v64) and np.array_equal(ruv, uv.astype(np.float64))
    assert rtex.tolist() == [[[0, 128, 255], [51, 255, 0]]]
    assert np.array_equal(rtex.reshape(-1, 3), meshing._uchar_colors(texf))


def test_vt_is_flipped_against_the_rows_of_the_texture(tmp_path):
    """texel (i, j) of a 2 x 4 (H x W) texture: vt = ((i + 0.5) / 4, 1 - (j + 0.5) / 2), so that the texture's first row
    is the top of OBJ's upward v axis"""
    from neuraludf_amd import meshing
    v = np.zeros((3, 3), dtype=np.float32)
    f = np.array([[0, 1, 2]])
    ij = np.array([[[0, 0], [3, 0], [1, 1]]])
    uv = (ij + 0.5) / [4, 2]
    tex = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    meshing.write_obj(tmp_path / "t.obj", v, f, uv, tex)
    vt = [ln.split()[1:] for ln in (tmp_path / "t.obj").read_text().splitlines() if ln.startswith("vt ")]
    assert [[float(x) for x in p] for p in vt] == [[0.125, 0.75], [0.875, 0.75], [0.375, 0.25]]
    _, _, ruv, rtex = meshing.read_obj(tmp_path / "t.obj")
    assert np.array_equal(ruv, uv) and np.array_equal(rtex, tex)
    # the texel a UV names, read the way a viewer does (v upwards): row (1 - vt.v) * H - 0.5
    for (i, j), (s, t) in zip(ij[0], [[float(x) for x in p] for p in vt]):
        assert (int(s * 4 - 0.5), int((1 - t) * 2 - 0.5)) == (i, j)


def test_refused_files(tmp_path):
    from neuraludf_amd import meshing
    v, f, uv, tex = _mesh()
    with pytest.raises(ValueError):
        meshing.write_obj(tmp_path / "x.obj", v, f, uv[:2], tex)
    with pytest.raises(ValueError):
        meshing.write_obj(tmp_path / "x.obj", v, f, uv, tex[..., 0])
    (tmp_path / "quad.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/1 4/1\n")
    with pytest.raises(ValueError, match="quad.obj:6"):
        meshing.read_obj(tmp_path / "quad.obj")
    (tmp_path / "far.obj").write_text("v 0 0 0\nvt 0 0\nf 1/1 2/1 1/1\n")
    with pytest.raises(ValueError, match="out of range"):
        meshing.read_obj(tmp_path / "far.obj")
    (tmp_path / "bare.obj").write_text("# no material\nv 0 0 0\nv 1 0 0\nv 1 1 0\nvt 0 0\nf 1/1 2/1 3/1\n")
    assert meshing.read_obj(tmp_path / "bare.obj")[3] is None
