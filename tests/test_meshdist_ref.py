"""CPU: the numpy restatement of the point-to-mesh rule (tests/meshdist_ref.py) against things it was not built from:
exact analytic cases, Ericson's region algorithm written separately in np.longdouble, and the rule's stated properties
(exact end points, winding independence, the (d2, face) order, barycentric weights that reproduce linear functions)."""
import numpy as np
import pytest

import meshdist_ref as R

TRI_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TRI_F = np.array([[0, 1, 2]])


@pytest.mark.parametrize("q, dist, point, bary", [
    ((0.25, 0.25, 2.0), 2.0, (0.25, 0.25, 0.0), (0.5, 0.25, 0.25)),        # interior
    ((-3.0, -4.0, 0.0), 5.0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)),            # v0
    ((0.5, -2.0, 0.0), 2.0, (0.5, 0.0, 0.0), (0.5, 0.5, 0.0)),             # edge 0-1
    ((1.0, 1.0, 0.0), np.sqrt(0.5), (0.5, 0.5, 0.0), (0.0, 0.5, 0.5)),     # the hypotenuse
])
def test_exact_analytic_cases(q, dist, point, bary):
    d, f, p, w = R.closest(np.array([q]), TRI_V, TRI_F)
    assert d[0] == dist and f[0] == 0
    assert p[0].tolist() == list(point) and w[0].tolist() == list(bary)


# ---- Ericson, Real-Time Collision Detection 5.1.5, in extended precision --------------------------------------------------
def _ericson(p, a, b, c):
    """closest point of triangle abc to p by Voronoi regions; every argument broadcastable [..., 3] np.longdouble"""
    def dot(x, y):
        return (x * y).sum(-1)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1 / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    full = np.broadcast_shapes(p.shape, a.shape)
    pts = [np.broadcast_to(a, full), np.broadcast_to(b, full), a + v_ab[..., None] * ab, np.broadcast_to(c, full),
           a + w_ac[..., None] * ac, b + w_bc[..., None] * (c - b)]
    out = a + ab * (vb * denom)[..., None] + ac * (vc * denom)[..., None]
    for cond, pt in zip(reversed(conds), reversed(pts)):              # the first region that matches wins
        out = np.where(cond[..., None], pt, out)
    return out


def _random_mesh(rng):
    """500 faces over 400 vertices in a box of side 4: random triangles, needles (aspect 1e-3) and near-degenerate
    faces (sin of the apex angle 1e-3 .. 1e-2).  The interior candidate's normal carries a relative direction error of
    about eps / sin(angle), so these bounds keep the rule's own error near 1e-13 L: the 1e-12 L asserted below is meant
    for such faces, not for exactly collinear ones (those are their edges, tested apart)."""
    v = rng.uniform(-2, 2, (400, 3))
    f = rng.integers(0, 400, (500, 3))
    f[f[:, 0] == f[:, 1], 1] = (f[f[:, 0] == f[:, 1], 0] + 1) % 400
    f[f[:, 2] == f[:, 0], 2] = (f[f[:, 2] == f[:, 0], 0] + 2) % 400
    f[f[:, 2] == f[:, 1], 2] = (f[f[:, 2] == f[:, 1], 1] + 3) % 400
    extra_v, extra_f = [], []
    for k in range(60):
        a = rng.uniform(-2, 2, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        o = np.cross(d, rng.normal(size=3))
        o /= np.linalg.norm(o)
        length = rng.uniform(0.2, 1.0)
        if k % 2:                                                      # a needle: a short third side
            tri = [a, a + length * d, a + length * 1e-3 * o]
        else:                                                          # nearly collinear: the apex close to the base
            tri = [a, a + length * d, a + 0.5 * length * d + length * rng.uniform(1e-3, 1e-2) * o]
        n0 = len(v) + len(extra_v)
        extra_v += tri
        extra_f.append([n0, n0 + 1, n0 + 2])
    v = np.concatenate([v, np.array(extra_v)])
    f[:60] = np.array(extra_f)
    return v, f


@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(11)
    v, f = _random_mesh(rng)
    q = rng.uniform(-2.5, 2.5, (2000, 3))
    q[:300] = v[f[rng.integers(0, len(f), 300)]].mean(1) + rng.normal(scale=1e-3, size=(300, 3))     # close to faces
    L = float(np.linalg.norm(v.max(0) - v.min(0)))
    return v, f, q, L, R.closest(q, v, f)


def test_against_ericson_in_extended_precision(random_case):
    v, f, q, L, (dist, face, point, bary) = random_case
    lv = v.astype(np.longdouble)
    A, B, C = (lv[f[:, k]][None] for k in range(3))
    ref_d = np.empty((len(q), len(f)), np.longdouble)
    for b in range(0, len(q), 250):
        P = q[b:b + 250].astype(np.longdouble)[:, None, :]
        c = _ericson(P, A, B, C)
        ref_d[b:b + 250] = np.sqrt(((P - c) ** 2).sum(-1))
    best = ref_d.min(1)
    err = np.abs(dist.astype(np.longdouble) - best).max()
    print("max |dist - ericson| / L = %.3g" % float(err / L))
    assert err <= 1e-12 * L
    # the winner is Ericson's, or a face as close within the tolerance
    assert (ref_d[np.arange(len(q)), face] - best).max() <= 1e-12 * L
    # the reported point is on the reported face at the reported distance, the weights are its coordinates
    blend = (bary[:, :, None] * v[f[face]]).sum(1)
    assert np.abs(blend - point).max() <= 1e-12 * L
    assert np.abs(np.linalg.norm(q - point, axis=1) - dist).max() <= 1e-12 * L
    assert (bary >= 0).all() and np.abs(bary.sum(1) - 1).max() <= 1e-12


def test_every_vertex_is_at_distance_zero(random_case):
    v, f = random_case[:2]
    used = np.unique(f)
    d, face, p, w = R.closest(v[used], v, f)
    assert (d == 0.0).all() and (p == v[used]).all()
    assert ((w == 0) | (w == 1)).all() and (w.sum(1) == 1).all()
    assert (f[face][w == 1] == used).all()


def test_winding_changes_no_distance_bit(random_case):
    v, f, q, _, (dist, face, point, _) = random_case
    d2, f2, p2, _ = R.closest(q, v, f[:, ::-1])
    assert d2.tobytes() == dist.tobytes() and (f2 == face).all()
    rolled = R.closest(q, v, np.roll(f, 1, axis=1))
    assert rolled[0].tobytes() == dist.tobytes()


def test_shared_edges_agree_to_the_bit():
    """two faces on one edge, listed in opposite directions: a query closest to that edge gets one d2 from both"""
    v = np.array([[0.1, 0.2, 0.3], [1.3, 0.9, 0.7], [0.4, 1.5, -0.2], [0.9, -0.8, 0.5]])
    # above the edge, off both faces' planes and outside both
    q = np.array([v[0] + t * (v[1] - v[0]) + 2.0 * np.cross(v[1] - v[0], v[2] - v[3]) for t in (0.2, 0.5, 0.9)])
    a = R.face_candidates(q, v, np.array([[0, 1, 2]]))[0]
    b = R.face_candidates(q, v, np.array([[1, 0, 3]]))[0]
    assert a.tobytes() == b.tobytes()


def test_duplicate_face_gives_the_lower_index(random_case):
    v, f, q = random_case[:3]
    f2 = np.concatenate([f, f[:50]])
    d, face, _, _ = R.closest(q[:400], v, f2)
    assert d.tobytes() == random_case[4][0][:400].tobytes()
    assert (face < len(f)).all() and (face == random_case[4][1][:400]).all()


def test_degenerate_and_absent_faces():
    v = np.array([[0.0, 0, 0], [2.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0], [5.0, 5, 5]])
    q = np.array([[1.0, 3.0, 0.0], [-1.0, 0.0, 0.0], [5.0, 5.0, 6.0]])
    d, face, p, w = R.closest(q, v, np.array([[0, 1, 2], [4, 4, 4], [0, 3, 1], [0, 1, 7]]))
    assert d.tolist() == [3.0, 1.0, 1.0] and face.tolist() == [0, 0, 1]
    assert p.tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [5.0, 5.0, 5.0]]
    assert w[2].tolist() == [1.0, 0.0, 0.0]
    d, face, p, w = R.closest(q, v, np.array([[0, 3, 1]]))                   # a NaN vertex: the face is absent
    assert np.isinf(d).all() and (face == -1).all() and np.isnan(p).all() and np.isnan(w).all()
    d, face, _, _ = R.closest(q, v, np.array([[0, 1, 2]]), bound=2.0)
    assert d.tolist() == [np.inf, 1.0, np.inf] and face.tolist() == [-1, 0, -1]


def test_linear_attribute_is_reproduced_where_the_distance_is_zero(random_case):
    v, f, _, L, _ = random_case
    rng = np.random.default_rng(5)
    G, c0 = rng.normal(size=(3, 4)), rng.normal(size=4)
    G /= np.abs(G).max()
    attr = v @ G + c0
    used = np.unique(f)
    mids = 0.5 * (v[f[:, 0]] + v[f[:, 1]])
    q = np.concatenate([v[used], mids])
    d, face, p, w = R.closest(q, v, f)
    zero = d == 0
    assert zero.sum() >= len(used)
    blend = (w[:, :, None] * attr[f[face]]).sum(1)
    assert np.abs(blend - (p @ G + c0))[zero].max() <= 1e-12 * L
