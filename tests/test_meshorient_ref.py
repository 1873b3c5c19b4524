"""CPU: the numpy restatement of the face orientation and the vertex normals (tests/meshorient_ref.py) pinned on meshes
whose answer is known: the restated mesher's N = 33 sphere (closed, orientable, two faces in five wound against the
rest), a Moebius band, the same band without the twist, the tie rule, and normals against closed forms and against
trimesh's arccos formula."""
import math

import numpy as np
import pytest

import meshorient_ref as O
import meshudf_ref as R

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def sphere():
    U, G, axes = R.sphere_grid(33, 0.6)
    v, f = R.marching_cubes(U, G, axes, *BOX)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def test_sphere_of_the_restated_mesher(sphere):
    v, f = sphere
    assert (len(v), len(f)) == (1758, 3512) and R.is_closed_manifold(f)
    edges = O.manifold_edges(f)
    assert len(edges) == 5268
    # a walk of our own over the same edges: the parity of every face against face 0
    par = {0: False}
    todo = [0]
    nbr = {}
    for a, b, same in edges:
        nbr.setdefault(a, []).append((b, same))
        nbr.setdefault(b, []).append((a, same))
    while todo:
        a = todo.pop()
        for b, same in nbr[a]:
            if b not in par:
                par[b] = par[a] ^ same
                todo.append(b)
    k = sum(par.values())
    assert len(par) == len(f)
    out, flipped, labels, orientable = O.orient(v, f)
    print(f"sphere: {int(flipped.sum())} of {len(f)} faces flipped, walk parity {k}")
    assert (labels == 0).all() and orientable.all()
    assert int(flipped.sum()) == min(k, len(f) - k) == 1472
    assert O.incompatible_edges(f) > 0 and O.incompatible_edges(out) == 0
    np.testing.assert_array_equal(out[~flipped], f[~flipped])
    np.testing.assert_array_equal(out[flipped], f[flipped][:, [0, 2, 1]])
    # outward from the centre: positive volume, radial normals
    out_c, flipped_c, _, _ = O.orient(v, f, outward_from=(0.0, 0.0, 0.0))
    assert O.incompatible_edges(out_c) == 0
    vol = O.signed_volume(v, out_c)
    print(f"signed volume {vol:.4f} (ideal sphere {4 / 3 * math.pi * 0.6 ** 3:.4f})")
    assert 0.89 < vol < 4 / 3 * math.pi * 0.6 ** 3
    assert (flipped_c == flipped).all() or (flipped_c == ~flipped).all()
    n = O.vertex_normals(v, out_c)
    radial = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    cos = np.einsum("ij,ij->i", n, radial)
    print(f"min cosine against radial {cos.min():.5f}")
    assert cos.min() >= 0.99
    raw = np.einsum("ij,ij->i", O.vertex_normals(v, f), radial)
    print(f"as meshed: {np.mean(raw > 0):.2f} of the vertex normals point outward, mean cosine {raw.mean():.2f}")
    assert np.mean(raw > 0) < 0.6
    assert O.signed_volume(v, out_c[:, [0, 2, 1]]) < 0


def test_moebius_band_is_left_alone():
    v, f = O.band(12, twist=True)
    assert f.shape == (24, 3) and f[-2:].tolist() == [[22, 1, 0], [22, 0, 23]]
    for origin in (None, (0.0, 0.0, 0.0)):
        out, flipped, labels, orientable = O.orient(v, f, origin)
        assert (labels == 0).all() and not orientable.any() and not flipped.any()
        np.testing.assert_array_equal(out, f)
    # it is the band that cannot be oriented, not the restatement: without one quad it can
    out, flipped, labels, orientable = O.orient(v, f[:-2])
    assert orientable.all() and (labels == 0).all() and O.incompatible_edges(out) == 0


def test_untwisted_band_needs_no_flip():
    v, f = O.band(12, twist=False)
    assert f[-2:].tolist() == [[22, 0, 1], [22, 1, 23]]
    out, flipped, labels, orientable = O.orient(v, f)
    assert orientable.all() and (labels == 0).all() and not flipped.any() and O.incompatible_edges(f) == 0
    np.testing.assert_array_equal(out, f)
    # a third of the faces turned over: exactly those are turned back
    g = f.copy()
    turned = np.random.default_rng(1).random(len(f)) < 1 / 3
    g[turned] = g[turned][:, [0, 2, 1]]
    out, flipped, _, _ = O.orient(v, g)
    assert 0 < turned.sum() < len(f) / 2 and (flipped == turned).all()
    np.testing.assert_array_equal(out, f)


def test_tie_and_the_edges_that_connect_nothing():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [2, 2, 2]], dtype=np.float64)
    f = np.array([[0, 1, 2], [1, 3, 2]])                               # edge 1-2 runs 1 -> 2 in one face and 2 -> 1 in the other
    out, flipped, labels, orientable = O.orient(v, f)
    assert not flipped.any() and labels.tolist() == [0, 0]
    alike = np.array([[0, 1, 2], [1, 2, 3]])                           # both run 1 -> 2: a tie, face 1 is flipped
    out, flipped, labels, orientable = O.orient(v, alike)
    assert flipped.tolist() == [False, True] and out.tolist() == [[0, 1, 2], [1, 3, 2]] and orientable.all()
    out, flipped, _, _ = O.orient(v, alike[::-1])
    assert flipped.tolist() == [False, True] and out.tolist() == [[1, 2, 3], [0, 2, 1]]
    # outward_from decides instead: seen from below (z < 0) the faces must run clockwise in the plane
    out, flipped, _, _ = O.orient(v, alike, outward_from=(0.3, 0.3, -1.0))
    assert O.incompatible_edges(out) == 0 and flipped.tolist() == [False, True]
    out, flipped, _, _ = O.orient(v, alike, outward_from=(0.3, 0.3, 1.0))
    assert flipped.tolist() == [True, False]
    out, flipped, _, _ = O.orient(v, alike, outward_from=(0.3, 0.3, 0.0))     # in the plane: S = 0, the first rule decides
    assert flipped.tolist() == [False, True]
    # three faces on one edge stay three components; a face with a repeated vertex is its own and is never flipped
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [3, 3, 1], [0, 3, 5]])
    out, flipped, labels, orientable = O.orient(v, fan, outward_from=(5.0, 5.0, 5.0))
    assert labels.tolist() == [0, 1, 2, 3, 1] and orientable.all() and not flipped[3]
    assert O.manifold_edges(fan) == [(1, 4, True)]
    out, flipped, labels, _ = O.orient(v, fan)
    assert flipped.tolist() == [False, False, False, False, True]
    # empty
    out, flipped, labels, orientable = O.orient(v, np.zeros((0, 3), dtype=np.int64))
    assert out.shape == (0, 3) and flipped.shape == labels.shape == orientable.shape == (0,)


def test_normals_closed_forms():
    # a regular tetrahedron wound outward: the normal at a vertex is its direction from the centre
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    f, _, _, _ = O.orient(v, f, outward_from=(0.0, 0.0, 0.0))
    assert O.signed_volume(v, f) > 0
    np.testing.assert_allclose(O.vertex_normals(v, f), v / math.sqrt(3.0), atol=1e-15)
    # a flat fan: every normal is +z whatever the angles; an unreferenced vertex and a face of zero area give zeros
    fan_v = np.array([[0, 0, 0], [2, 0, 0], [1, 3, 0], [-1, 0.5, 0], [-0.5, -2, 0], [9, 9, 9], [4, 0, 0]], dtype=np.float64)
    fan_f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 6]])
    n = O.vertex_normals(fan_v, fan_f)
    np.testing.assert_array_equal(n[:5], np.tile([0.0, 0.0, 1.0], (5, 1)))
    np.testing.assert_array_equal(n[5:], np.zeros((2, 3)))
    # angle weights: two faces that meet along the edge 0-1; vertex 0 sees 90 degrees of each, vertex 2 45 of the first
    roof_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 1]], dtype=np.float64)
    roof_f = np.array([[0, 1, 2], [0, 3, 1]])
    n = O.vertex_normals(roof_v, roof_f)
    n1 = np.cross(roof_v[3] - roof_v[0], roof_v[1] - roof_v[0])
    want = math.pi / 2 * np.array([0.0, 0.0, 1.0]) + math.pi / 2 * n1 / np.linalg.norm(n1)
    np.testing.assert_allclose(n[0], want / np.linalg.norm(want), atol=1e-15)
    want2 = math.pi / 4 * np.array([0.0, 0.0, 1.0])                   # vertex 2 is used by the first face only
    np.testing.assert_allclose(n[2], want2 / np.linalg.norm(want2), atol=1e-15)


def test_normals_equal_the_arccos_formula(sphere):
    v, f = sphere
    out, _, _, _ = O.orient(v, f, outward_from=(0.0, 0.0, 0.0))
    np.testing.assert_allclose(O.vertex_normals(v, out), O.vertex_normals_arccos(v, out), rtol=0, atol=1e-12)
    for twist in (True, False):
        bv, bf = O.band(12, twist=twist)
        n, length = O.vertex_normals(bv, bf, return_length=True)
        assert length.min() > 0.05                         # no vertex whose sum cancels: the two formulas' roundings stay small
        np.testing.assert_allclose(n, O.vertex_normals_arccos(bv, bf), rtol=0, atol=1e-12)
