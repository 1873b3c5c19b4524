"""CPU: PLY files with vertex colours (meshing.write_ply colors=, read_ply with_colors=): the round trip with colours, with
normals and colours, and with neither -- and the file written without colours is, byte for byte, what write_ply wrote
before it learnt about colours (a copy of that function is kept here)."""
import numpy as np
import pytest


def write_ply_before(path, vertices, faces, normals=None):
    """meshing.write_ply as it was before the `colors` argument"""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f4").reshape(-1, 3))
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        nrm = np.asarray(normals, dtype="<f4").reshape(-1, 3)
        if len(nrm) != len(v):
            raise ValueError("vertices and normals differ in length")
        v = np.ascontiguousarray(np.concatenate([v, nrm], 1))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    f = np.asarray(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("face index out of range")
    rec = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"], rec["v"] = 3, f
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), props, len(f)))
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def _mesh():
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((7, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=np.int64)
    normals = rng.standard_normal((7, 3)).astype(np.float32)
    colors = rng.random((7, 3)).astype(np.float32)
    colors[0], colors[1] = (0.0, 1.0, 0.5), (-0.2, 1.3, 0.49999)         # the ends, a tie and values to clip
    return verts, faces, normals, colors


def _uchar(c):
    return np.rint(np.clip(np.asarray(c, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


@pytest.mark.parametrize("with_normals", [False, True])
def test_round_trip_with_colours(tmp_path, with_normals):
    from neuraludf_amd import meshing
    verts, faces, normals, colors = _mesh()
    path = tmp_path / "c.ply"
    meshing.write_ply(path, verts, faces, normals if with_normals else None, colors)
    v, f, n, c = meshing.read_ply(path, with_normals=True, with_colors=True)
    assert np.array_equal(v, verts.astype(np.float64)) and np.array_equal(f, faces)
    assert (n is None) != with_normals and (n is None or np.array_equal(n, normals.astype(np.float64)))
    assert c.dtype == np.uint8 and np.array_equal(c, _uchar(colors))
    assert list(c[0]) == [0, 255, 128] and list(c[1]) == [0, 255, 127]
    head = path.read_bytes().split(b"end_header\n")[0].decode()
    names = [ln.split()[-1] for ln in head.splitlines() if ln.startswith("property") and "list" not in ln]
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + ["red", "green", "blue"]
    assert "property uchar red" in head
    # uint8 colours pass through, and the readers that do not ask for colours see the same mesh
    meshing.write_ply(path, verts, faces, None, _uchar(colors))
    assert np.array_equal(meshing.read_ply(path, with_colors=True)[2], _uchar(colors))
    v2, f2 = meshing.read_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    with pytest.raises(ValueError):
        meshing.write_ply(path, verts, faces, None, colors[:-1])


@pytest.mark.parametrize("with_normals", [False, True])
def test_without_colours_the_file_is_what_it_was(tmp_path, with_normals):
    from neuraludf_amd import meshing
    verts, faces, normals, _ = _mesh()
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    meshing.write_ply(a, verts, faces, normals if with_normals else None)
    write_ply_before(b, verts, faces, normals if with_normals else None)
    assert a.read_bytes() == b.read_bytes()
    out = meshing.read_ply(a, with_normals=True, with_colors=True)
    assert len(out) == 4 and out[3] is None and (out[2] is None) != with_normals
    assert len(meshing.read_ply(a)) == 2 and len(meshing.read_ply(a, with_normals=True)) == 3


def test_ascii_colours(tmp_path):
    from neuraludf_amd import meshing
    path = tmp_path / "t.ply"
    path.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
                    "property list uchar int vertex_indices\nend_header\n0 0 0 255 0 7\n1 0 0 1 2 3\n0 1 0 9 8 7\n3 0 1 2\n")
    v, f, c = meshing.read_ply(path, with_colors=True)
    assert c.dtype == np.uint8 and c.tolist() == [[255, 0, 7], [1, 2, 3], [9, 8, 7]] and f.tolist() == [[0, 1, 2]]
