"""CPU checks of the MeshUDF mesher's pieces that need no GPU: the generated marching-cubes table
(neuraludf_amd/mc_tables.py, committed as csrc/mc_tables.inc), the numpy restatement of the mesher on an analytic grid
and the PLY writer.  (The ABI mirror of NudfMeshUDF: tests/test_abi.py.)"""
import collections

import numpy as np
import pytest

from neuraludf_amd import mc_tables as T
from neuraludf_amd import meshing

import meshudf_ref as R

TABLE = T.tables()


def _on_face(face):
    return set(T.face_edges(face))


@pytest.mark.parametrize("case", range(256))
def test_case_triangulation(case):
    tris = TABLE[case]
    change = set(T.sign_change_edges(case))
    used = {e for t in tris for e in t}
    assert used <= change                      # only sign-change edges
    assert used == change                      # and every one of them
    assert all(len(set(t)) == 3 for t in tris)
    count = collections.Counter(frozenset(p) for t in tris for p in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])))
    faces = [_on_face(f) for f in T.FACES]
    for seg, n in count.items():
        on_a_face = any(seg <= fe for fe in faces)
        assert n == (1 if on_a_face else 2), (case, sorted(seg), n)     # internal edges: exactly 2 triangles
    for f, fe in zip(T.FACES, faces):
        left = {seg for seg in count if seg <= fe}
        assert left == {frozenset(s) for s in T.face_segments(case, f)}, (case, f)


def test_face_rule_keeps_plus_corners_connected():
    # corners 0 and 3 `-`, on a diagonal of the x = 0 face (corners 0, 2, 3, 1 in cyclic order): each is cut off alone
    face = T.FACES[0]
    assert face[:2] == (0, 0) and face[2] == [0, 2, 3, 1]
    segs = {frozenset(s) for s in T.face_segments((1 << 0) | (1 << 3), face)}
    assert segs == {frozenset((T.edge_of(0, 2), T.edge_of(0, 1))), frozenset((T.edge_of(3, 2), T.edge_of(3, 1)))}


def test_triangles_face_the_plus_side():
    for case in range(1, 255):
        for t in TABLE[case]:
            p = [np.array([(T.CORNERS[a][x] + T.CORNERS[b][x]) / 2 for x in range(3)]) for a, b in (T.EDGES[e] for e in t)]
            normal = np.cross(p[1] - p[0], p[2] - p[0])
            to_plus = sum((np.array(T.CORNERS[b]) - T.CORNERS[a]) * (1 if case >> a & 1 else -1)
                          for a, b in (T.EDGES[e] for e in t))
            assert normal @ to_plus > 0, (case, t)


def test_committed_table_is_the_generators_output():
    with open(T.INC_PATH) as f:
        assert f.read() == T.render_inc()


def test_restatement_sphere_is_a_closed_surface():
    n, radius = 33, 0.6
    U, G, axes = R.sphere_grid(n, radius)
    verts, faces = R.marching_cubes(U, G, axes, (-1, -1, -1), (1, 1, 1))
    assert len(faces) > 0
    assert R.is_closed_manifold(faces)
    assert R.euler(len(verts), faces) == 2
    assert R.components(len(verts), faces) == 1
    h = meshing.grid_spacing((-1, -1, -1), (1, 1, 1), n)
    assert np.abs(np.linalg.norm(verts, axis=1) - radius).max() < 0.05 * h


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (5, 3)).astype(np.int64)
    path = tmp_path / "m.ply"
    meshing.write_ply(str(path), v, f)
    data = path.read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert "element vertex 7" in head and "element face 5" in head
    assert "property list uchar int vertex_indices" in head
    body = data[end:]
    v2 = np.frombuffer(body[:7 * 12], dtype="<f4").reshape(7, 3)
    rec = np.frombuffer(body[7 * 12:], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    np.testing.assert_array_equal(v2, v)
    assert (rec["n"] == 3).all() and len(rec) == 5
    np.testing.assert_array_equal(rec["v"], f)
    with pytest.raises(ValueError):
        meshing.write_ply(str(path), v, f + 7)
