"""CPU: the numpy restatement of the mesh clean-up (tests/meshclean_ref.py) against independent statements of the same
things -- scipy's connected components, the reference's literal sparse-matrix smoothing and matmul projection, scipy's
binary dilation -- and hand-built cases; plus the host-side footprint and dilation of neuraludf_amd.meshclean."""
import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import meshclean_ref as M
import meshudf_ref as R
from neuraludf_amd import meshclean

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
OCTA = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


@pytest.fixture(scope="module")
def sphere():
    U, G, axes = R.sphere_grid(33, 0.6)
    return R.marching_cubes(U, G, axes, *BOX)


def _scipy_labels(faces, n_verts):
    """smallest face index per component of the face-adjacency graph (faces sharing an undirected edge), by scipy"""
    edges, he_edge = M.edge_table(faces, n_verts)
    face = np.arange(len(he_edge)) // 3
    order = np.argsort(he_edge, kind="stable")
    same = he_edge[order][1:] == he_edge[order][:-1]
    a, b = face[order][:-1][same], face[order][1:][same]
    g = coo_matrix((np.ones(len(a)), (a, b)), shape=(len(faces), len(faces)))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, len(faces))
    np.minimum.at(first, lab, np.arange(len(faces)))
    return first[lab]


def test_edge_table_counts_and_faces():
    edges, he_edge = M.edge_table(TETRA[:3], 4)
    uniq, cnt = R.edge_counts(TETRA[:3])
    np.testing.assert_array_equal(edges[:, :2], uniq)
    np.testing.assert_array_equal(edges[:, 2], cnt)
    for e, (u, v, c, f0, f1) in enumerate(edges):
        users = [i for i, t in enumerate(TETRA[:3]) if u in t and v in t]
        assert users[:2] == [x for x in (f0, f1) if x >= 0] and len(users) == c
    for h, e in enumerate(he_edge):
        t = TETRA[h // 3]
        assert sorted((t[h % 3], t[(h % 3 + 1) % 3])) == list(edges[e, :2])
    np.testing.assert_array_equal(M.boundary_degree(TETRA[:3], 4), [2, 0, 2, 2])


def test_components_against_scipy_random_soups():
    rng = np.random.default_rng(1)
    for n_verts, n_faces in [(12, 10), (40, 30), (200, 150), (60, 200)]:
        f = np.stack([rng.permutation(n_verts)[:3] for _ in range(n_faces)])
        np.testing.assert_array_equal(M.face_components(f, n_verts), _scipy_labels(f, n_verts))


def test_components_two_disjoint_spheres(sphere):
    v, f = sphere
    f2 = np.concatenate([f, f + len(v)])
    lab = M.face_components(f2, 2 * len(v))
    np.testing.assert_array_equal(lab, _scipy_labels(f2, 2 * len(v)))
    assert set(lab.tolist()) == {0, len(f)}
    vv, ff = M.filter_components(np.concatenate([v, v + 3]), f2[:-7], keep_largest=True)
    np.testing.assert_array_equal(ff, f)
    np.testing.assert_array_equal(vv, v)
    vv, ff = M.filter_components(np.concatenate([v, v + 3]), f2, keep_largest=True)      # tie: the smallest label
    np.testing.assert_array_equal(ff, f)


def test_smoothing_against_the_literal_expression(sphere):
    v, f = sphere
    keep = np.ones(len(f), dtype=bool)
    keep[M.remove_disjoint_faces(f, 20)] = False
    f20 = f[keep]
    lit = M.smooth_borders_literal(v, f20)
    mine = M.smooth_borders(v, f20, dtype=np.float64)
    assert (M.boundary_degree(f20, len(v)).max()) == 2
    np.testing.assert_array_equal(mine, lit)                   # two neighbours per border vertex: bit-equal
    assert (mine != v.astype(np.float64)).any(1).sum() == 60
    # a border vertex with four boundary edges (two fans touching in vertex 0): 1e-12 relative
    fans = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]])
    pts = np.random.default_rng(2).normal(size=(7, 3))
    assert M.boundary_degree(fans, 7)[0] == 4
    a, b = M.smooth_borders(pts, fans, dtype=np.float64), M.smooth_borders_literal(pts, fans)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    np.testing.assert_array_equal(M.smooth_borders(pts, TETRA, dtype=np.float64), pts)     # closed: nothing moves


def test_footprint():
    np.testing.assert_array_equal(meshclean.ellipse_footprint(5),
                                  [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]])
    fp = meshclean.ellipse_footprint(11)
    spans = [(int(np.nonzero(r)[0][0]), int(np.nonzero(r)[0][-1]) + 1) for r in fp]
    assert spans[:6] == [(5, 6), (2, 9), (1, 10), (0, 11), (0, 11), (0, 11)]
    for k in (11, 31):
        fp = meshclean.ellipse_footprint(k)
        assert fp.shape == (k, k) and fp.dtype == np.uint8
        np.testing.assert_array_equal(fp, fp[::-1])
        np.testing.assert_array_equal(fp, fp[:, ::-1])
        for r in fp:                                           # every row is one run
            c = np.nonzero(r)[0]
            assert len(c) and len(c) == c[-1] - c[0] + 1
    with pytest.raises(ValueError):
        meshclean.ellipse_footprint(0)


def test_dilation_against_scipy():
    rng = np.random.default_rng(4)
    m = (rng.random((3, 40, 57)) > 0.97).astype(np.uint8) * 255
    m[0, 0, 0] = m[1, -1, -1] = m[2, 0, -1] = 255                   # corners: the border handling
    for k in (1, 3, 5, 11, 31):
        fp = meshclean.ellipse_footprint(k)
        want = np.stack([ndimage.binary_dilation(x != 0, structure=fp) for x in m]).astype(np.uint8)
        np.testing.assert_array_equal(M.dilate(m, fp), want)
        got = meshclean.dilate_masks(torch.from_numpy(m), k, chunk=2)
        assert got.dtype == torch.uint8
        np.testing.assert_array_equal(got.numpy(), want)


def test_fill_tetrahedron_minus_a_face():
    f, n = M.fill_holes(TETRA_V, TETRA[:3])
    assert n == 1
    np.testing.assert_array_equal(f, TETRA)                         # the removed face, in its winding
    assert R.is_closed_manifold(f)
    f3, n3 = M.fill_holes(TETRA_V, TETRA[:3], max_loop=3)
    np.testing.assert_array_equal(f3, TETRA)


def test_fill_octahedron_minus_two_adjacent_faces():
    f, n = M.fill_holes(OCTA_V, OCTA[2:])
    assert n == 1 and len(f) == 8
    np.testing.assert_array_equal(f[6:], [[0, 2, 4], [1, 4, 2]])    # split along 2-4 (sqrt 2), not 0-1 (2); OCTA's winding
    assert R.is_closed_manifold(f) and R.euler(6, f) == 2
    f3, n3 = M.fill_holes(OCTA_V, OCTA[2:], max_loop=3)
    assert n3 == 0 and len(f3) == 6
    # equal diagonals: the one through the smallest index
    pyramid = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])
    pv = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], dtype=np.float64)
    f, n = M.fill_holes(pv, pyramid)
    assert n == 1
    np.testing.assert_array_equal(f[4:], [[0, 2, 1], [0, 3, 2]])
    assert R.is_closed_manifold(f)


def test_fill_leaves_touching_loops_long_loops_and_existing_triangles():
    two = np.array([[0, 1, 3], [1, 2, 3], [2, 0, 3], [0, 4, 6], [4, 5, 6], [5, 0, 6]])     # 3-loops 0-1-2 and 0-4-5
    v = np.random.default_rng(5).normal(size=(7, 3))
    assert M.boundary_degree(two, 7)[0] == 4
    f, n = M.fill_holes(v, two)
    assert n == 0 and len(f) == 6
    five = np.array([[i, (i + 1) % 5, 5] for i in range(5)])
    f, n = M.fill_holes(v[:6], five)
    assert n == 0 and len(f) == 5
    one = np.array([[0, 1, 2]])
    f, n = M.fill_holes(v[:3], one)
    assert n == 0 and len(f) == 1
    f, n = M.fill_holes(v[:3], np.zeros((0, 3), dtype=np.int64))
    assert n == 0 and f.shape == (0, 3)


def test_fill_restores_removed_sphere_faces(sphere):
    v, f = sphere
    gone = M.remove_disjoint_faces(f, 20)
    keep = np.ones(len(f), dtype=bool)
    keep[gone] = False
    assert R.boundary_loops(len(v), f[keep]) == (60, 20)
    filled, n = M.fill_holes(v, f[keep])
    assert n == 20 and len(filled) == len(f)
    new = filled[len(f) - 20:]
    want = np.sort(f[gone], 1)
    np.testing.assert_array_equal(np.sort(new, 1), want[np.argsort(want[:, 0], kind="stable")])
    assert R.is_closed_manifold(filled) and R.euler(len(v), filled) == 2
    assert (new[:, 0] == new.min(1)).all()


def test_projection_equals_the_literal_matmul_on_the_rig(sphere):
    """the fixed-order row sums give the same integer pixels as the reference's np.matmul expression for every vertex
    and view of the rig: no vertex sits within an ulp of a half pixel at this seed"""
    v, _ = sphere
    pts = v.astype(np.float64) * M.RIG_SCALE
    mats, masks = M.camera_rig()
    assert masks.shape == (8, 300, 400)
    for P in mats:
        mine = M.project_pixels(pts, P)
        assert np.isfinite(mine).all()
        np.testing.assert_array_equal(mine.astype(np.int32), M.project_pixels_literal(pts, P))
    cnt = M.view_counts(pts, mats, masks)
    assert 0 < (cnt > 2).sum() < len(pts) and len(set(cnt.tolist())) >= 4         # the rig separates the vertices


def test_view_counts_hand_computed():
    W, H = 16, 8
    P = np.array([[[4.0, 0, 8, 0], [0, 4, 4, 0], [0, 0, 1, 0], [0, 0, 0, 1]]])       # u = 4 x / z + 8, v = 4 y / z + 4
    mask = np.zeros((1, H, W), dtype=np.uint8)
    mask[0, 4, 8] = mask[0, 4, 10] = mask[0, 4, 15] = 1
    pts = np.array([[0, 0, 1],           # (8, 4) -> pixel (9, 5): mask[4, 8]
                    [0.125, 0, 1],       # u = 8.5 -> 8 (half to even) -> 9: mask[4, 8]; rounding up would hit mask[4, 9] = 0
                    [0.375, 0, 1],       # u = 9.5 -> 10 -> 11: mask[4, 10]; rounding down would hit mask[4, 9] = 0
                    [1.75, 0, 1],        # u = 15 -> x = 16 = W: the last column inside, mask[4, 15]
                    [2, 0, 1],           # u = 16 -> x = 17 = W + 1: out
                    [0, 0, -1],          # behind the camera: (8, 4) again; the reference has no depth test
                    [1, 1, 0],           # z = 0: inf
                    [0, 0, 0],           # z = 0: nan
                    [-2.25, 0, 1],       # u = -1 -> x = 0: the padding column of ones
                    [0, 0.25, 1]],       # (8, 5) -> pixel (9, 6): mask[5, 8] = 0
                   dtype=np.float64)
    np.testing.assert_array_equal(M.view_counts(pts, P, mask), [1, 1, 1, 1, 0, 1, 0, 0, 1, 0])
    np.testing.assert_array_equal(M.view_counts(pts, P, mask, border=2), [1, 1, 1, 0, 0, 1, 0, 0, 0, 0])
    faces = np.array([[0, 1, 2], [0, 3, 4], [5, 8, 3]])
    v, f = M.clean_by_views(pts, faces, P, mask, "mask", minimal_vis=0)
    assert len(v) == 6 and f.tolist() == [[0, 1, 2], [4, 5, 3]]             # unreferenced survivors stay
    v, f = M.clean_by_views(pts, faces[:2], P, mask, "mask", minimal_vis=0)
    assert len(v) == 6 and f.tolist() == [[0, 1, 2]]
    v, f = M.clean_by_views(pts, faces[:2], P, mask, "mask", minimal_vis=0, drop_unreferenced=True)
    assert len(v) == 3 and f.tolist() == [[0, 1, 2]]
    v, f = M.clean_by_views(pts, np.array([[0, 1, 2], [3, 4, 8]]), P, mask, "hull", max_outside=1, border=2)
    assert len(v) == 6 and f.tolist() == [[0, 1, 4]]                        # keeps the vertices counted 0 times


def test_compact_keeps_order():
    v = np.arange(18, dtype=np.float64).reshape(6, 3)
    f = np.array([[0, 1, 2], [2, 3, 5], [1, 2, 5]])
    vv, ff = M.compact(v, f, face_mask=np.array([False, True, True]))
    np.testing.assert_array_equal(vv, v[[1, 2, 3, 5]])
    assert ff.tolist() == [[1, 2, 3], [0, 1, 3]]
    vv, ff = M.compact(v, f, vertex_mask=np.array([1, 1, 1, 0, 1, 1], bool), drop_unreferenced=False)
    np.testing.assert_array_equal(vv, v[[0, 1, 2, 4, 5]])
    assert ff.tolist() == [[0, 1, 2], [1, 2, 4]]
