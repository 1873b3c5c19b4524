"""CPU: properties of the subdivision rules (include/nudf.h), on the numpy restatement alone
(tests/meshsubdiv_ref.py): what the midpoint and edge-length splits must leave unchanged, what Loop's scheme must and must
not move, and the four face templates by hand."""
import math

import numpy as np
import pytest

import meshray_ref
import meshsmooth_ref
import meshsubdiv_ref as R

MESHES = R.meshes()
NAMES = sorted(MESHES)
MANIFOLD = [n for n in NAMES if n != "awkward"]          # awkward_mesh: coincident vertices and repeated corners
RATIOS = (0.75, 0.3, 0.07)


def _longest(v, f):
    return R.longest_edge(v, R.edge_table(f, len(v)))


@pytest.fixture(scope="module")
def to_edge():
    """subdivide_to_edge of every mesh at every ratio, once"""
    out = {}
    for name, (v, f) in MESHES.items():
        for ratio in RATIOS:
            out[name, ratio] = R.subdivide_to_edge(v, f, ratio * _longest(v, f))
    return out


@pytest.fixture(scope="module")
def uniform():
    return {(name, scheme): R.subdivide_mesh(v, f, 1, scheme) for name, (v, f) in MESHES.items() for scheme in R.SCHEMES}


# ---- midpoint and edge-length splits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_area_is_unchanged(name, to_edge, uniform):
    v, f = MESHES[name]
    a0 = R.area(v, f)
    for s in [uniform[name, "midpoint"]] + [to_edge[name, r] for r in RATIOS]:
        assert abs(R.area(s.verts, s.faces) - a0) <= 1e-12 * a0
        np.testing.assert_array_equal(s.verts[:len(v)], v)                     # the old vertices keep index and place


@pytest.mark.parametrize("name", MANIFOLD)
def test_counts_scale_as_they_must(name, to_edge, uniform):
    v, f = MESHES[name]
    V, E, F, hist = R.euler(v, f)
    for scheme in R.SCHEMES:
        s = uniform[name, scheme]
        want = {c: 2 * n for c, n in hist.items()}                                 # an old edge becomes two of its kind
        want[2] = want.get(2, 0) + 3 * F                                           # and every face gets three inside it
        assert R.euler(s.verts, s.faces) == (V + E, 2 * E + 3 * F, 4 * F, want)
        assert len(s.verts) == len(v) + E and s.rounds == 1 and s.converged
        np.testing.assert_array_equal(s.parent_face, np.repeat(np.arange(F), 4))
    for ratio in RATIOS:
        s = to_edge[name, ratio]
        V1, E1, F1, hist1 = R.euler(s.verts, s.faces)
        assert V1 - E1 + F1 == V - E + F                                           # the Euler characteristic
        assert set(hist1) <= set(hist) | {2}                                       # new edges lie inside faces: two sides
        assert all(hist1[c] >= hist[c] for c in hist if c != 2)                    # a split edge keeps its face count


@pytest.mark.parametrize("name", NAMES)
def test_rounds_and_longest_edge(name, to_edge):
    v, f = MESHES[name]
    L = _longest(v, f)
    for ratio in RATIOS:
        s = to_edge[name, ratio]
        assert s.converged and s.longest_edge <= ratio * L
        assert s.longest_edge == _longest(s.verts, s.faces)
        assert s.rounds == R.expected_rounds(L, ratio * L) == math.ceil(math.log2(1.0 / ratio))
        assert s.parent_face.shape == (len(s.faces),) and (np.diff(s.parent_face) >= 0).all()
    capped = R.subdivide_to_edge(v, f, 0.07 * L, max_rounds=2)
    assert not capped.converged and capped.rounds == 2
    assert 0.07 * L < capped.longest_edge <= 0.07 * L + (L - 0.07 * L) / 4.0       # the bound after k rounds
    assert R.subdivide_to_edge(v, f, 2.0 * L).rounds == 0


@pytest.mark.parametrize("name", NAMES)
def test_children_keep_the_winding(name, to_edge, uniform):
    v, f = MESHES[name]
    n0 = R.face_normals(v, f)
    for s in [uniform[name, "midpoint"]] + [to_edge[name, r] for r in RATIOS]:
        n1 = R.face_normals(s.verts, s.faces)
        assert ((n1 * n0[s.parent_face]).sum(1) >= 0.0).all()
        assert s.faces.min() >= 0 and s.faces.max() < len(s.verts)


def test_attributes_follow_the_positions():
    v, f = MESHES["sheet"]
    for scheme in R.SCHEMES:
        s = R.subdivide_mesh(v, f, 2, scheme, attributes=v[:, [2, 0, 1]].copy())
        np.testing.assert_array_equal(s.attributes, s.verts[:, [2, 0, 1]])
    s = R.subdivide_to_edge(v, f, 0.3 * _longest(v, f), attributes=v.copy())
    np.testing.assert_array_equal(s.attributes, s.verts)


# ---- Loop ---------------------------------------------------------------------------------------------------------------
def test_loop_keeps_a_flat_sheet_flat():
    v, f = meshray_ref.grid_sheet(6)
    s = R.subdivide_mesh(np.array(v, np.float64), f, 2, "loop")
    assert (s.verts[:, 2] == 0.0).all() and np.abs(s.verts[:len(v)] - v).max() > 1e-3


def test_loop_holds_a_crease():
    v, f = MESHES["three"]
    s = R.subdivide_mesh(v, f, 1, "loop")
    np.testing.assert_array_equal(s.verts[:2], v[:2])
    assert (np.abs(s.verts[2:5] - v[2:5]).max(1) > 1e-3).all()
    t = R.edge_table(f, len(v))
    e01 = int(np.nonzero((t.u == 0) & (t.v == 1))[0][0])
    np.testing.assert_array_equal(s.verts[len(v) + e01], (v[0] + v[1]) * 0.5)   # a crease edge gets its midpoint


def test_loop_rounds_a_sphere():
    v, f = meshray_ref.icosphere(1)

    def spread(x):
        r = np.linalg.norm(x, axis=1)
        return (r.max() - r.min()) / r.mean()
    loop, mid = (spread(R.subdivide_mesh(v, f, 2, s).verts) for s in ("loop", "midpoint"))
    print(f"icosphere(1), two levels: radial spread loop {loop:.3g}, midpoint {mid:.3g}")
    assert loop < 0.5 * mid


def test_loop_smooths_a_noisy_sheet():
    v, f, _ = meshsmooth_ref.noisy_sheet()
    def angle(pos, faces):
        """mean angle in degrees of the unit face normals (meshsmooth_ref.frames) to the z axis"""
        return meshsmooth_ref.mean_normal_angle(meshsmooth_ref.frames(pos, faces)[0], np.tile([0.0, 0.0, 1.0], (len(faces), 1)))
    before = angle(v, f)
    out = {scheme: angle(*R.subdivide_mesh(v, f, 1, scheme)[:2]) for scheme in R.SCHEMES}
    print(f"noisy_sheet: mean normal angle {before:.2f} -> loop {out['loop']:.2f}, midpoint {out['midpoint']:.2f}")
    assert out["loop"] < 0.75 * before and out["midpoint"] == before            # midpoint: bit for bit
    # midpoint: every child lies in its parent's plane
    s = R.subdivide_mesh(v, f, 1, "midpoint")
    n0 = R.face_normals(v, f)
    n1 = R.face_normals(s.verts, s.faces)
    cos = (n1 * n0[s.parent_face]).sum(1) / (np.linalg.norm(n1, axis=1) * np.linalg.norm(n0[s.parent_face], axis=1))
    assert cos.min() > 1.0 - 1e-12


def test_loop_weights_sum_to_one():
    """a constant attribute stays constant to rounding, whatever the valence and the class of the vertex"""
    for name in NAMES:
        v, f = MESHES[name]
        s = R.subdivide_mesh(v, f, 1, "loop", attributes=np.full((len(v), 1), 3.0))
        assert np.abs(s.attributes - 3.0).max() <= 4 * 3.0 * 2.0 ** -52, name


# ---- the templates by hand ---------------------------------------------------------------------------------------------------
QUAD_V = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
QUAD_F = np.array([(0, 1, 2), (0, 2, 3)], np.int64)
# the edges of the quad in table order: (0,1) (0,2) (0,3) (1,2) (2,3)
E01, E02, E03, E12, E23 = range(5)


def _split(marked, verts=QUAD_V, faces=QUAD_F):
    t = R.edge_table(faces, len(verts))
    assert list(zip(t.u.tolist(), t.v.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (2, 3)]
    marks = np.zeros(5, bool)
    marks[list(marked)] = True
    n, pos, out, _, parent = R.one_round(verts, faces, None, "midpoint", marks=marks)
    assert n == len(marked)
    return pos, out.tolist(), parent.tolist()


def test_template_none_and_one():
    pos, faces, parent = _split([E01])
    np.testing.assert_array_equal(pos[4], [1.0, 0.0, 0.0])
    assert faces == [[0, 4, 2], [4, 1, 2], [0, 2, 3]] and parent == [0, 0, 1]
    pos, faces, parent = _split([E02])                      # the shared edge: both faces split it, 4 = its midpoint
    np.testing.assert_array_equal(pos[4], [1.0, 0.5, 0.0])
    assert faces == [[2, 4, 1], [4, 0, 1], [0, 4, 3], [4, 2, 3]] and parent == [0, 0, 1, 1]


def test_template_two_takes_the_shorter_diagonal():
    # face (0, 1, 2) with (1, 2) and (2, 0) marked: a = 0, b = 1, c = 2, m1 = 5 on (1, 2), m2 = 4 on (0, 2)
    pos, faces, parent = _split([E02, E12])
    np.testing.assert_array_equal(pos[4:], [[1.0, 0.5, 0.0], [2.0, 0.5, 0.0]])
    # |a - m1|^2 = 4.25 > |b - m2|^2 = 1.25: along b - m2
    assert faces[:3] == [[5, 2, 4], [0, 1, 4], [1, 5, 4]] and parent == [0, 0, 0, 1, 1]
    assert faces[3:] == [[0, 4, 3], [4, 2, 3]]
    # a wide corner at b instead: a - m1 is the shorter one
    v = QUAD_V.copy()
    v[1] = [0.2, -3.0, 0.0]
    pos, faces, _ = _split([E02, E12], v)
    assert R._dist2(pos[0], pos[5]) < R._dist2(pos[1], pos[4])
    assert faces[:3] == [[5, 2, 4], [0, 1, 5], [0, 5, 4]]


def test_template_two_tie():
    # an isosceles face: both diagonals are medians of equal length; a < b decides for a - m1, and b < a against
    v = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    for f, want in (([(0, 1, 2)], [[4, 2, 3], [0, 1, 4], [0, 4, 3]]), ([(1, 0, 2)], [[3, 2, 4], [1, 0, 4], [0, 3, 4]])):
        f = np.array(f, np.int64)
        t = R.edge_table(f, 3)
        assert list(zip(t.u.tolist(), t.v.tolist())) == [(0, 1), (0, 2), (1, 2)]
        n, pos, out, _, parent = R.one_round(v, f, None, "midpoint", marks=[False, True, True])
        assert R._dist2(pos[0], pos[4]) == R._dist2(pos[1], pos[3])
        assert out.tolist() == want and parent.tolist() == [0, 0, 0]


def test_template_three():
    pos, faces, parent = _split([E01, E02, E12])
    # new vertices in edge order: 4 on (0, 1), 5 on (0, 2), 6 on (1, 2)
    assert faces[:4] == [[0, 4, 5], [4, 1, 6], [5, 6, 2], [4, 6, 5]]
    assert faces[4:] == [[0, 5, 3], [5, 2, 3]] and parent == [0, 0, 0, 0, 1, 1]


def test_degenerate_faces_stay_valid():
    v, f = MESHES["awkward"]
    for scheme in R.SCHEMES:
        s = R.subdivide_mesh(v, f, 2, scheme)
        assert s.faces.min() >= 0 and s.faces.max() < len(s.verts) and np.isfinite(s.verts).all()
        rep = (s.faces[:, 0] == s.faces[:, 1]) | (s.faces[:, 1] == s.faces[:, 2]) | (s.faces[:, 2] == s.faces[:, 0])
        f0 = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
        assert rep.any() and f0[s.parent_face[rep]].all()                  # degenerate in, degenerate out, and only there
    t = R.edge_table(f, len(v))
    assert not R.mark(v, t)[t.u == t.v].any() and (t.u == t.v).any()
    nan = v.copy()
    nan[0, 0] = np.nan
    assert not R.mark(nan, t, 1e-3)[(t.u == 0) | (t.v == 0)].any()             # a NaN length is not marked
