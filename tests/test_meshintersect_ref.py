"""CPU: the restatement of the intersection rule (tests/meshintersect_ref.py, which the GPU kernels must equal bit for bit)
against something it was not built from: a closed triangle / triangle intersection in exact rational arithmetic
(fractions.Fraction) -- plane signs, then the points where an edge of one meets the other, the corners of one inside the
other and the crossings of coplanar edges, which together hold every corner of the common set.  For faces that share
vertices it asks for a common point outside the hull of the shared vertices (the vertex; the edge).  For every pair the
narrow phase is handed: not reported => exactly disjoint, CROSSING => exactly intersecting.  No tolerance."""
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import meshintersect_cases as cases
import meshintersect_ref as R
import meshray_ref


# ---- the exact test ------------------------------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _normal(t):
    n = _cross(_sub(t[1], t[0]), _sub(t[2], t[0]))
    assert any(n), "the exact test needs triangles with an area"
    return n


def _inside(p, t, n):
    """p in the closed triangle t of normal n"""
    if _dot(_sub(p, t[0]), n) != 0:
        return False
    return all(_dot(_cross(_sub(t[(k + 1) % 3], t[k]), _sub(p, t[k])), n) >= 0 for k in range(3))


def _common_points(t1, t2):
    """points of both closed triangles, among them every corner of their common set"""
    out = []
    for s, t in ((t1, t2), (t2, t1)):
        n = _normal(t)
        h = [_dot(_sub(p, t[0]), n) for p in s]
        out += [p for p, hp in zip(s, h) if hp == 0 and _inside(p, t, n)]
        for k in range(3):
            a, b, ha, hb = s[k], s[(k + 1) % 3], h[k], h[(k + 1) % 3]
            if ha * hb < 0:
                w = ha / (ha - hb)
                p = tuple(a[x] + w * (b[x] - a[x]) for x in range(3))
                if _inside(p, t, n):
                    out.append(p)
    for k in range(3):                                       # edges that cross in one point, neither end in the other's plane
        p, u = t1[k], _sub(t1[(k + 1) % 3], t1[k])
        for l in range(3):
            q, w = t2[l], _sub(t2[(l + 1) % 3], t2[l])
            c, d = _cross(u, w), _sub(q, p)
            cc = _dot(c, c)
            if cc == 0 or _dot(d, c) != 0:
                continue
            s, t = _dot(_cross(d, w), c) / cc, _dot(_cross(d, u), c) / cc
            if 0 <= s <= 1 and 0 <= t <= 1:
                out.append(tuple(p[x] + s * u[x] for x in range(3)))
    return out


def exact_intersects(c1, c2, shared=()):
    """the closed triangles share a point outside the hull of `shared` (no, one or two of their corners, as points)"""
    t1 = [tuple(Fraction(float(x)) for x in p) for p in c1]
    t2 = [tuple(Fraction(float(x)) for x in p) for p in c2]
    n = _normal(t2)
    h = [_dot(_sub(p, t2[0]), n) for p in t1]
    if all(x > 0 for x in h) or all(x < 0 for x in h):
        return False
    sh = [tuple(Fraction(float(x)) for x in p) for p in shared]
    for p in _common_points(t1, t2):
        if len(sh) == 0:
            return True
        if len(sh) == 1 and p != sh[0]:
            return True
        if len(sh) == 2:
            e, d = _sub(sh[1], sh[0]), _sub(p, sh[0])
            if any(_cross(e, d)) or not 0 <= _dot(d, e) <= _dot(e, e):
                return True
    return False


def check_against_exact(verts, faces, other=None):
    """the two implications for every handed pair -> Counter of the kinds"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    vb, fb = (verts, faces) if other is None else (np.asarray(other[0], np.float64), np.asarray(other[1], np.int64))
    kinds = Counter()
    for a, b, kind in R.tested(verts, faces, other):
        kinds[kind] += 1
        if kind not in (R.NONE, R.CROSSING):
            continue
        shared = sorted(set(faces[a].tolist()) & set(fb[b].tolist())) if other is None else []
        if len(shared) == 3:
            assert kind == R.NONE
            continue
        hit = exact_intersects(verts[faces[a]], vb[fb[b]], verts[shared])
        assert hit == (kind == R.CROSSING), (a, b, kind, hit)
    return kinds


# ---- the inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_triangles(seed):
    """300 triangles in the unit cube, edges about 0.2.  At most 1 % of the pairs whose boxes overlap may be COPLANAR or
    UNCERTAIN: a condition on the filter, which must decide generic input.  Measured: 0 of 349, 0 of 307 and 0 of 298 for
    the seeds 0, 1 and 2."""
    verts, faces = R.random_triangles(300, 0.2, seed)
    kinds = check_against_exact(verts, faces)
    n = sum(kinds.values())
    print("pairs", n, dict(kinds))
    assert n > 200 and kinds[R.CROSSING] > 20
    assert kinds[R.COPLANAR] + kinds[R.UNCERTAIN] <= 0.01 * n


def test_two_spheres_merged_and_as_two_meshes():
    a, b = R.two_spheres(2, 0.3)
    verts, faces = R.merged(a, b)
    kinds = check_against_exact(verts, faces)
    assert kinds[R.CROSSING] > 50 and kinds[R.COPLANAR] + kinds[R.UNCERTAIN] == 0
    fa = len(a[1])                                             # as two meshes: the same pairs, checked above
    assert R.pairs(a[0], a[1], other=b) == [(x, y - fa, k) for x, y, k in R.pairs(verts, faces)]
    # every crossing pair lies across the two spheres: a sphere does not cross itself
    assert all(x < fa <= y for x, y, _ in R.pairs(verts, faces))


def test_sphere_alone_reports_nothing():
    verts, faces = meshray_ref.icosphere(2)
    kinds = check_against_exact(verts, faces)
    assert set(kinds) == {R.NONE} and kinds[R.NONE] > 1000


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_cases(name):
    verts, faces, want = cases.HAND[name]
    assert R.pairs(verts, faces) == want
    finite = np.isfinite(verts[faces]).all((1, 2))
    check_against_exact(np.nan_to_num(verts), faces[finite])


def test_spiked_sheet_crosses_only_where_the_patch_would_go():
    verts, faces, _, _ = cases.spiked_sheet()
    assert R.pairs(verts, faces) == []                      # the spike stands in the hole and touches nothing yet
    check_against_exact(verts, faces)


def test_relabelled_vertices_and_rotated_corners_change_nothing():
    a, b = R.two_spheres(1, 0.3)
    verts, faces = R.merged(a, b)
    want = R.pairs(verts, faces)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(verts))
    inv = np.argsort(perm)
    rolled = np.stack([np.roll(f, k) for f, k in zip(faces, rng.integers(0, 3, len(faces)))])
    assert R.pairs(verts[perm], inv[rolled]) == want


@pytest.mark.parametrize("mesh", ["random", "spheres", "sheet"])
def test_broad_phase_hands_each_pair_once_whatever_the_cell(mesh):
    if mesh == "random":
        verts, faces = R.random_triangles(300, 0.2, 0)
    elif mesh == "spheres":
        verts, faces = R.merged(*R.two_spheres(2, 0.3))
    else:
        verts, faces = cases.spiked_sheet()[:2]
    corners, ok = R.usable_corners(verts, faces)
    want = R.box_pairs(corners, ok, corners, ok, True)
    cell = R.default_cell(verts, faces)
    for factor in (0.5, 1.0, 4.0):
        got = R.handed(verts, faces, factor * cell)
        assert len(got) == len(set(got)), factor
        assert sorted(got) == want, factor
