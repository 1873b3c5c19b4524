"""CPU: the numpy restatement of the texture atlas (tests/meshtexture_ref.py) pinned on facts that need no GPU, before the
GPU tests compare the kernels against it: the chart geometry inside a cell, the packing of random class mixes, and the
layout of a scene worked out by hand."""
import numpy as np
import pytest

import meshraster_scenes as S
import meshtexture_ref as T


@pytest.mark.parametrize("s", [8, 16, 32])
def test_every_bilinear_footprint_stays_on_the_charts_own_texels(s):
    """the 2 x 2 taps of any point of a chart (corners, edges and a dense sample of the inside) lie in the cell and belong
    to the chart's own half; both charts are counter-clockwise right isosceles triangles, with legs of s - 5 (lower) and s - 6
    (upper) texels"""
    t = np.linspace(0.0, 1.0, 4 * s + 1)
    a, b = np.meshgrid(t, t, indexing="ij")
    keep = a + b <= 1.0 + 1e-12
    a, b = a[keep], b[keep]
    for half, chart in enumerate((T.lower_chart(s), T.upper_chart(s))):
        c = np.asarray(chart, dtype=np.float64)
        e1, e2 = c[1] - c[0], c[2] - c[0]
        assert e1[0] * e2[1] - e1[1] * e2[0] > 0 and e1 @ e2 == 0 and abs(e1).sum() == abs(e2).sum() == s - 5 - half
        pts = c[0] + a[:, None] * e1 + b[:, None] * e2
        for dx in (0, 1):
            for dy in (0, 1):                                    # the taps of a point: floor and floor + 1
                i, j = np.floor(pts[:, 0]).astype(int) + dx, np.floor(pts[:, 1]).astype(int) + dy
                assert i.min() >= 0 and j.min() >= 0 and i.max() <= s - 1 and j.max() <= s - 1
                assert {T.owner_half(x, y, s) for x, y in zip(i, j)} == {half}
    assert sum(T.owner_half(i, j, s) == 0 for i in range(s) for j in range(s)) == s * (s + 1) // 2


def test_morton_packing_of_random_class_mixes_never_overlaps():
    rng = np.random.default_rng(0)
    for _ in range(50):
        n_classes = int(rng.integers(1, 5))
        ks = sorted(rng.choice(np.arange(3, 9), n_classes, replace=False).tolist(), reverse=True)
        cells = rng.integers(1, 6, n_classes).tolist()
        off = [0]
        for k, n in zip(ks, cells):
            off.append(off[-1] + n * 4 ** k)
        W = 1
        while W * W < off[-1]:
            W *= 2
        H = W // 2 if off[-1] <= W * W // 2 else W
        used = np.zeros((H, W), dtype=np.int32)
        for c, (k, n) in enumerate(zip(ks, cells)):
            for e in range(n):
                m0 = off[c] + e * 4 ** k
                X, Y = T.even_bits(m0), T.even_bits(m0 >> 1)
                assert X % (1 << k) == 0 and Y % (1 << k) == 0
                used[Y:Y + (1 << k), X:X + (1 << k)] += 1        # (a slice past the atlas would come up short: caught below)
        assert used.max() == 1 and used.sum() == off[-1]


def test_layout_of_the_two_squares_by_hand():
    """density 8: the large square's faces (longest edge 2 sqrt 2 -> 22.6 texels) need 2^5 - 6 = 26, the small one's (0.707
    -> 5.66) 2^4 - 6 = 10: one cell of side 32 at (0, 0), one of side 16 at Morton offset 1024 = (32, 0); 2 x 1024 texels
    fill the lower half of a 64 x 64 square: 64 x 32"""
    v, f = S.two_squares()
    lay = T.layout(v, f, 8.0)
    assert lay["k"].tolist() == [5, 5, 4, 4] and lay["class_k"] == (5, 4) and lay["class_off"] == (0, 1024, 1280)
    assert (lay["W"], lay["H"]) == (64, 32) and lay["cell_face"].tolist() == [[0, 1], [2, 3]]
    # face 0 = (0, 1, 2): its longest edge is the diagonal 0-2, opposite corner 1, which sits at the right angle (1, 1)
    assert lay["uv"][0].tolist() == [[1, 28], [1, 1], [28, 1]]
    # face 1 = (0, 2, 3): the diagonal is opposite corner 2 (vertex 3): the upper chart's right angle (30, 30)
    assert lay["uv"][1].tolist() == [[4, 30], [30, 4], [30, 30]]
    assert lay["uv"][2].tolist() == [[33, 12], [33, 1], [44, 1]] and lay["uv"][3].tolist() == [[36, 14], [46, 4], [46, 14]]
    own = T.owners(lay, 4)
    assert own.shape == (32, 64) and (own == 0).sum() == 32 * 33 // 2 and (own == 1).sum() == 32 * 31 // 2
    assert (own == 2).sum() == 16 * 17 // 2 and (own == -1).sum() == 64 * 32 - 1280
    assert own[0, 0] == 0 and own[31, 31] == 1 and own[0, 32] == 2 and own[15, 47] == 3 and own[16, 32] == -1


def test_degenerate_faces_take_the_smallest_cell_and_long_ones_the_largest():
    v, f, _, _ = S.ragged()
    n = len(f)
    k = T.layout(v, f, 1e5)["k"]
    assert k[n - 1] == 3 and k[n - 2] == 3                       # the NaN vertex, the repeated vertex
    assert k[n - 3] == 12 and np.all(k[:n - 2] == 12)            # the collinear face has edges: it is sized like any other
    assert np.all(T.layout(v, f, 1e-6)["k"] == 3)
    bad = np.concatenate([f, [[0, 1, len(v)]]])                  # a vertex index out of range
    assert T.layout(v, bad, 1e5)["k"][-1] == 3
