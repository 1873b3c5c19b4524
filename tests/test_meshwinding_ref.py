"""CPU: the numpy restatement of the winding-number kernels (tests/meshwinding_ref.py) held to things it was not built
from: solid angles known in closed form, closed meshes, an independent brute-force sum, moments summed directly about the
node's centre, the measured error of the expansion (DESIGN.md 4.22 quotes this test's figures; run with -s to see them),
and the reason for the feature: a sphere with holes that the crossing parity gets wrong and the winding number gets right.

Measured here (max |w_beta - w_inf| over 1 500 random points in the mesh's box grown by a quarter of its longest side):
    beta   sphere (320)   two sheets (1024)   Moebius (384)   fan (288)   punched sphere (1178)
    1.5    2.3e-3         1.2e-2              2.3e-3          1.2e-3      3.7e-3
    2      7.6e-4         2.7e-3              5.5e-4          2.8e-4      1.2e-3
    3      9.1e-5         3.0e-4              6.0e-5          2.4e-5      1.4e-4
    4      1.7e-5         7.5e-5              1.7e-5          0           4.3e-5
At beta = 2 a query evaluates 70 / 12 / 14 / 272 / 34 faces exactly and 31 / 29 / 19 / 1 / 50 nodes by expansion on
average.  The smallest | |w| - 0.5 | of the containment fixtures is 0.367 (the punched sphere); the worst error of the
default on any of these meshes is 2.7e-3."""
import functools

import numpy as np
import pytest

import meshray_ref
import meshwinding_ref as R

BETAS = (1.5, 2.0, 3.0, 4.0)
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "sphere":
        return meshray_ref.icosphere(2)
    if name == "sheets":
        return R.two_sheets(16)
    if name == "moebius":
        return R.moebius()
    if name == "fan":
        return R.fan()
    if name == "cube":
        return meshray_ref.cube()
    if name == "punched":
        return R.punched_sphere()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _tree(name):
    return R.Tree(*_mesh(name))


def _box_points(name, n, seed, grow=0.25):
    v = _mesh(name)[0]
    lo, hi = v.min(0), v.max(0)
    pad = grow * (hi - lo).max()
    return np.random.default_rng(seed).uniform(lo - pad, hi + pad, (n, 3))


def test_one_triangle_is_an_eighth_of_the_sky():
    v = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    for f in ([0, 1, 2], [0, 2, 1]):
        w = R.winding(R.Tree(v, np.array([f])), np.zeros((1, 3)), np.inf)
        assert abs(abs(w["w"][0]) - 0.125) < 4 * U and w["exact"][0] == 1 and w["far"][0] == 0
    # in the face's plane, at a vertex, on the face: exactly 0, no sign of zero decides
    q = np.array([[2.0, -1.0, 0.0], [1.0, 0, 0], [1 / 3, 1 / 3, 1 / 3], [0.5, 0.5, 0.0]])
    q[2] = (v[0] + (v[1] + v[2])) / 3.0
    got = R.winding(R.Tree(v, np.array([[0, 1, 2]])), q[[0, 1, 3]], np.inf)["w"]
    assert (got == 0).all()


@pytest.mark.parametrize("name", ["cube", "sphere"])
def test_closed_meshes_give_one_inside_and_zero_outside(name):
    v, f = _mesh(name)
    scale = 0.5 if name == "cube" else 1.0
    rng = np.random.default_rng(1)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    inside, outside = d * (0.6 * scale) * rng.uniform(0, 1, (200, 1)), d * (2.5 * scale) * rng.uniform(1, 4, (200, 1))
    tree = _tree(name)
    win, wout = R.winding(tree, inside, np.inf), R.winding(tree, outside, np.inf)
    tol = 4 * len(f) * U * np.maximum(1.0, np.r_[win["abs"], wout["abs"]]).max()
    assert np.abs(win["w"] - 1.0).max() <= tol and np.abs(wout["w"]).max() <= tol
    assert (win["exact"] == len(f)).all() and (win["far"] == 0).all()


def test_a_hemisphere_covers_half_the_sky_from_the_centre():
    """latitude rings from the equator (z = 0 exactly) to the pole: the border lies in a plane through the centre, so the
    cap covers 2 pi whatever its tessellation"""
    rings, seg = 6, 24
    lon = np.arange(seg) * (2 * np.pi / seg)
    v = [(np.cos(a), np.sin(a), 0.0) for a in lon]
    for k in range(1, rings):
        lat = k * (np.pi / 2) / rings
        v += [(np.cos(lat) * np.cos(a), np.cos(lat) * np.sin(a), np.sin(lat)) for a in lon]
    v.append((0.0, 0.0, 1.0))
    f = []
    for k in range(rings - 1):
        for s in range(seg):
            a, b = k * seg + s, k * seg + (s + 1) % seg
            f += [(a, b, b + seg), (a, b + seg, a + seg)]
    f += [((rings - 1) * seg + s, (rings - 1) * seg + (s + 1) % seg, len(v) - 1) for s in range(seg)]
    r = R.winding(R.Tree(np.array(v), np.array(f)), np.zeros((1, 3)), np.inf)
    assert abs(r["w"][0] - 0.5) <= 4 * len(f) * U and r["exact"][0] == len(f)


@pytest.mark.parametrize("name", ["sphere", "sheets", "moebius", "fan"])
@pytest.mark.parametrize("beta", [2.0, np.inf])
def test_flipping_every_face_negates_w_bit_for_bit(name, beta):
    v, f = _mesh(name)
    q = _box_points(name, 200, 2)
    a, b = R.winding(_tree(name), q, beta), R.winding(R.Tree(v, f[:, [0, 2, 1]]), q, beta)
    assert np.array_equal(a["w"], -b["w"]) and np.array_equal(a["exact"], b["exact"]) and np.array_equal(a["far"], b["far"])


@pytest.mark.parametrize("name", ["sphere", "sheets", "moebius", "fan", "punched"])
def test_beta_inf_is_the_brute_force_sum(name):
    """the two sum the same terms in different orders: n terms re-rounded n - 1 times each way"""
    v, f = _mesh(name)
    q = _box_points(name, 300, 3)
    got = R.winding(_tree(name), q, np.inf)
    want = R.brute(v, f, q)
    assert (got["exact"] == len(f)).all() and (got["far"] == 0).all()
    bound = 2 * len(f) * U * got["abs"] + 1e-300
    assert (np.abs(got["w"] - want) <= bound).all(), np.abs(got["w"] - want).max()


def test_absent_faces_change_nothing():
    v, f = _mesh("sphere")
    v2, f2 = R.with_absent_faces(v, f)
    t1 = _tree("sphere")
    t2 = R.Tree(v2, f2, leaf=t1.leaf)                 # the two faces without an area still count in the mean box side
    assert t2.n_nodes == t1.n_nodes and np.array_equal(t2.sorted_faces, t1.sorted_faces + 3)
    assert (t2.face_keys[:3] == -1).all() and (t2.face_keys[3:] >= 0).all()
    q = _box_points("sphere", 100, 4)
    assert np.array_equal(R.winding(t2, q, 2.0)["w"], R.winding(t1, q, 2.0)["w"])


@pytest.mark.parametrize("name", ["sphere", "sheets", "moebius", "fan", "punched"])
def test_tree_is_a_preorder_and_moments_equal_direct_sums(name):
    v, f = _mesh(name)
    t = _tree(name)
    n, idx = t.n_nodes, np.arange(t.n_nodes)
    assert t.level[0] == t.level.max() and t.first[0] == 0 and t.end[0] == len(t.sorted_faces) and t.skip[0] == n
    assert (np.diff(t.first) >= 0).all() and (t.skip > idx).all() and (t.is_leaf == (t.level == 0)).all()
    ok, P, A, a, c = R.face_geometry(v, f)
    B = np.linalg.norm(t.hi - t.lo)
    for i in range(n):
        # a node's subtree is the nodes up to skip[i]: their faces are its faces
        assert t.first[i:t.skip[i]].min() == t.first[i] and t.end[i:t.skip[i]].max() == t.end[i]
        if t.skip[i] < n:
            assert t.first[t.skip[i]] == t.end[i]
        fs = t.sorted_faces[t.first[i]:t.end[i]]
        W = a[fs].sum()
        centre = (a[fs, None] * c[fs]).sum(0) / W
        rec = t.rec[i]
        nf = len(fs)
        assert np.abs(rec[0:3] - centre).max() <= 8 * nf * U * B
        delta = c[fs] - rec[0:3]
        S = A[fs].sum(0)
        T = np.einsum("fj,fk->jk", delta, A[fs])
        d = P[fs] - c[fs][:, None, :]
        C = np.einsum("fcj,fck->fjk", d, d) / 12.0
        Q = np.einsum("fi,fjk->ijk", A[fs], delta[:, :, None] * delta[:, None, :] + C)
        # raw sums about the box's corner: every partial sum is below W B^p and is rounded nf + a few times
        assert np.abs(rec[4:7] - S).max() <= 8 * nf * U * W
        assert np.abs(t.T[i] - T).max() <= 16 * nf * U * W * B
        assert np.abs(rec[7:10] - np.diag(T)).max() <= 16 * nf * U * W * B and abs(rec[31] - np.trace(T)) <= 48 * nf * U * W * B
        assert np.abs(rec[10:13] - (T + T.T)[[0, 0, 1], [1, 2, 2]]).max() <= 32 * nf * U * W * B
        for i3 in range(3):
            for (j, k), p in R.SYM.items():
                assert abs(rec[13 + 6 * i3 + p] - Q[i3, j, k]) <= 32 * nf * U * W * B * B
        pts = P[fs].reshape(-1, 3)
        assert np.array_equal(t.box_lo[i], pts.min(0)) and np.array_equal(t.box_hi[i], pts.max(0))
        far = np.maximum(rec[0:3] - pts.min(0), pts.max(0) - rec[0:3])
        assert rec[3] == R.dot3(*far) and rec[3] >= ((pts - rec[0:3]) ** 2).sum(1).max() * (1 - 8 * U)


@functools.lru_cache(maxsize=None)
def _expansion_errors(name):
    q = _box_points(name, 1500, 5)
    exact = R.winding(_tree(name), q, np.inf)["w"]
    out = {}
    for beta in BETAS:
        r = R.winding(_tree(name), q, beta)
        out[beta] = (np.abs(r["w"] - exact).max(), r["exact"].mean(), r["far"].mean())
    return out


def _containment_fixtures():
    """(name, points, inside) of the fixtures that contains_points is tested on: points well off the surface"""
    sphere_in, sphere_out = R.shell_points(2, 1.0, (0.5, 0.8)), R.shell_points(2, 1.0, (1.25,))
    yield "sphere", np.concatenate([sphere_in, sphere_out]), np.r_[np.ones(len(sphere_in), bool), np.zeros(len(sphere_out), bool)]
    pin, pout = R.shell_points(2, 0.6, (0.5, 0.8)), R.shell_points(2, 0.6, (1.25,))
    yield "punched", np.concatenate([pin, pout]), np.r_[np.ones(len(pin), bool), np.zeros(len(pout), bool)]


def test_expansion_error_falls_with_beta_and_stays_below_the_containment_margin(capsys):
    worst_default = 0.0
    for name in ("sphere", "sheets", "moebius", "fan", "punched"):
        err = _expansion_errors(name)
        with capsys.disabled():
            print("\n%-8s" % name + "  ".join("beta %g: %.2e (%.0f exact, %.0f far)" % ((b,) + err[b]) for b in BETAS))
        for lo, hi in zip(BETAS[:-1], BETAS[1:]):
            assert err[hi][0] <= err[lo][0], (name, lo, hi, err)
            assert err[hi][1] >= err[lo][1], (name, lo, hi, err)           # a larger beta opens more leaves
        worst_default = max(worst_default, err[2.0][0])
    margin = np.inf
    for name, pts, inside in _containment_fixtures():
        err = np.abs(R.winding(_tree(name), pts, 2.0)["w"] - R.winding(_tree(name), pts, np.inf)["w"]).max()
        worst_default = max(worst_default, err)
        margin = min(margin, np.abs(np.abs(R.winding(_tree(name), pts, np.inf)["w"]) - 0.5).min())
    with capsys.disabled():
        print("default beta: worst error %.2e, smallest margin %.3f" % (worst_default, margin))
    assert worst_default < margin


def test_the_winding_number_is_right_where_the_parity_is_wrong():
    """a sphere of 1 280 faces with 8 % of them removed: a ray can leave through a hole"""
    from neuraludf_amd import evaluation
    name, pts, inside = list(_containment_fixtures())[1]
    v, f = _mesh(name)
    assert len(f) == 1280 - 102
    parity = meshray_ref.parity_inside(pts, v, f, np.array(evaluation.INSIDE_DIRECTIONS))
    assert (parity != inside).sum() >= 1                       # 5 of the 324 inside points on this seed
    w = R.winding(_tree(name), pts, evaluation.WINDING_BETA)["w"]
    assert np.array_equal(np.abs(w) > 0.5, inside)
    assert w[inside].min() > 0.85 and np.abs(w[~inside]).max() < 0.1
    assert evaluation.WINDING_LEAF_FACTOR == R.WINDING_LEAF_FACTOR
