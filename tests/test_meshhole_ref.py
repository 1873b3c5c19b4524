"""CPU: the numpy restatement of the hole closing (tests/meshhole_ref.py) against brute force and against hand-built meshes.
The GPU tests hold csrc/meshhole.hip to this restatement bit for bit; here the restatement itself is held to the
definitions: the dynamic programme to the enumeration of every triangulation, the loop extraction through pointer doubling
to a plain walk along the links and to the loops the meshes were built with."""
import numpy as np
import pytest

import meshhole_cases as cases
import meshhole_ref as ref


def _triangulations(i, j):
    """every triangulation of v_i ... v_j as a list of (i, k, j), k ascending, the left part varying slowest"""
    if j - i < 2:
        yield []
        return
    for k in range(i + 1, j):
        for left in _triangulations(i, k):
            for right in _triangulations(k, j):
                yield [(i, k, j)] + left + right


def _total(P, tris, i, j):
    """the area of a triangulation summed in the dynamic programme's association: (left + right) + A"""
    if j - i < 2:
        return 0.0
    (a, k, b), rest = tris[0], tris[1:]
    n_left = max(k - i - 1, 0)
    return (_total(P, rest[:n_left], i, k) + _total(P, rest[n_left:], k, j)) + ref.area(P[a], P[k], P[b])


@pytest.mark.parametrize("n", range(3, 9))
def test_minimum_area_against_brute_force(n):
    rng = np.random.default_rng(100 + n)
    for _ in range(4):
        t = np.sort(rng.uniform(0, 2 * np.pi, n))
        P = np.stack([np.cos(t), np.sin(t), rng.standard_normal(n)], 1).tolist()
        W, split = ref.min_area(P)
        best, arg = None, None
        for tris in _triangulations(0, n - 1):
            total = _total(P, tris, 0, n - 1)
            if best is None or total < best:                  # the first strictly smaller total wins
                best, arg = total, tris
        got = ref.preorder(split, n)
        assert len(got) == n - 2
        assert W[0][n - 1] == best
        assert got == arg


def test_preorder_is_triangle_then_left_then_right():
    split = [[0] * 6 for _ in range(6)]
    split[0][5], split[0][3], split[3][5], split[0][2] = 3, 2, 4, 1
    assert ref.preorder(split, 6) == [(0, 3, 5), (0, 2, 3), (0, 1, 2), (3, 4, 5)]


def _loops(verts, faces):
    tb = ref.table(faces, len(verts))
    lnk = ref.link(faces, tb)
    walked = ref.loops(tb, lnk)
    ranked = ref.loops_from_rank(tb, lnk, ref.rank(lnk))
    for a, b in zip(walked, ranked):
        assert np.array_equal(a, b)
    # the link pairs the states
    s = np.arange(len(lnk))
    assert np.array_equal(lnk[lnk[lnk >= 0]], s[lnk >= 0])
    return tb, lnk, walked


def _lengths(lp, closed):
    n = np.diff(lp.loop_off)
    return sorted(n[lp.closed == closed].tolist())


def _check_canonical(tb, lp):
    """ids by smallest border edge; a closed loop starts with that edge at its smaller vertex and its edges chain up"""
    smallest = [lp.loop_edge[lp.loop_off[l]:lp.loop_off[l + 1]].min() for l in range(len(lp.closed))]
    assert smallest == sorted(smallest)
    for l in range(len(lp.closed)):
        e, v = lp.loop_edge[lp.loop_off[l]:lp.loop_off[l + 1]], lp.loop_vertex[lp.loop_off[l]:lp.loop_off[l + 1]]
        assert np.all(lp.edge_loop[e] == l)
        nxt = tb.u[e] + tb.v[e] - v                               # the other end of each edge
        assert np.array_equal(nxt[:-1], v[1:])
        if lp.closed[l]:
            assert e[0] == e.min() and v[0] == tb.u[e[0]] and nxt[-1] == v[0]
    assert (lp.edge_loop >= 0).sum() == len(lp.loop_edge) == (tb.count == 1).sum()


@pytest.mark.parametrize("k", (3, 4, 5, 7))
def test_disc_with_a_k_gon_hole(k):
    verts, faces = cases.annulus(k)
    tb, _, lp = _loops(verts, faces)
    assert _lengths(lp, True) == [k, k] and _lengths(lp, False) == []
    _check_canonical(tb, lp)
    hole = lp.edge_loop[np.nonzero((tb.count == 1) & (tb.v < k))[0]]
    assert len(set(hole.tolist())) == 1
    assert set(lp.loop_vertex[lp.loop_off[hole[0]]:lp.loop_off[hole[0] + 1]].tolist()) == set(range(k))


def test_bow_tie_comes_apart_into_two_loops():
    verts, faces = cases.bow_tie(4, 5)
    tb, _, lp = _loops(verts, faces)
    assert _lengths(lp, True) == [4, 4, 5, 5] and _lengths(lp, False) == []
    _check_canonical(tb, lp)
    with_shared = [l for l in range(4) if 0 in lp.loop_vertex[lp.loop_off[l]:lp.loop_off[l + 1]]]
    assert sorted(np.diff(lp.loop_off)[with_shared].tolist()) == [4, 5]
    for l in with_shared:                                       # each passes the shared vertex once
        assert (lp.loop_vertex[lp.loop_off[l]:lp.loop_off[l + 1]] == 0).sum() == 1
    st = ref.close_holes(verts, faces).status
    assert np.all(st == ref.FILLED)


def test_holes_pinched_in_one_sheet_are_one_loop_through_the_vertex_twice():
    verts, faces = cases.pinched_holes()
    tb, _, lp = _loops(verts, faces)
    assert _lengths(lp, True) == [8, 20] and _lengths(lp, False) == []
    _check_canonical(tb, lp)
    eight = int(np.nonzero(np.diff(lp.loop_off) == 8)[0][0])
    assert (lp.loop_vertex[lp.loop_off[eight]:lp.loop_off[eight + 1]] == 2 * 6 + 2).sum() == 2
    out = ref.close_holes(verts, faces)
    assert out.status[eight] == ref.REPEATED_VERTEX and not np.any(out.new_face_loop == eight)


def test_edge_with_three_faces_gives_open_chains():
    verts, faces = cases.fin()
    tb, lnk, lp = _loops(verts, faces)
    assert _lengths(lp, True) == [] and _lengths(lp, False) == [2, 4, 20]
    _check_canonical(tb, lp)
    assert (lnk < 0).sum() == 6                                 # two blocked ends per chain
    for l in range(3):                                          # a chain starts at the smaller of its two end states
        e, v = lp.loop_edge[lp.loop_off[l]:lp.loop_off[l + 1]], lp.loop_vertex[lp.loop_off[l]:lp.loop_off[l + 1]]
        first = 2 * tb.brank[e[0]] + (v[0] == tb.v[e[0]])
        last_exit = tb.u[e[-1]] + tb.v[e[-1]] - v[-1]
        last = 2 * tb.brank[e[-1]] + (last_exit == tb.v[e[-1]])
        assert lnk[first] < 0 and lnk[last] < 0 and first < last
    st = ref.close_holes(verts, faces).status
    assert np.all(st == ref.OPEN_CHAIN)


def test_face_with_a_repeated_vertex_blocks():
    verts, faces = cases.repeated_vertex_face()
    tb, lnk, lp = _loops(verts, faces)
    assert _lengths(lp, True) == [20] and _lengths(lp, False) == [1, 3]
    one = int(np.nonzero(np.diff(lp.loop_off) == 1)[0][0])
    e = lp.loop_edge[lp.loop_off[one]]
    assert tb.u[e] == tb.v[e] == 7 and np.all(lnk[2 * tb.brank[e]:2 * tb.brank[e] + 2] < 0)


def test_flipping_half_the_faces_changes_no_loop():
    for verts, faces in (cases.annulus(7), cases.bow_tie(), cases.fin(), cases.sphere_patch((3, 5, 6, 17))):
        _, lnk, lp = _loops(verts, faces)
        _, lnk2, lp2 = _loops(verts, cases.flip_half(faces))
        assert np.array_equal(lnk, lnk2)
        for a, b in zip(lp, lp2):
            assert np.array_equal(a, b)


def test_sphere_patch_has_the_holes_it_was_built_with():
    verts, faces = cases.sphere_patch()
    tb, _, lp = _loops(verts, faces)
    assert _lengths(lp, True) == sorted(cases.SPHERE_HOLES + (2 * (60 + 28),)) and _lengths(lp, False) == []
    _check_canonical(tb, lp)
    assert len(faces) <= 4000


def test_close_holes_restated():
    verts, faces = cases.sphere_patch()
    out = ref.close_holes(verts, faces, max_edges=64)
    n = np.diff(out.loops.loop_off)
    assert np.array_equal(out.status == ref.FILLED, n <= 64)
    assert np.all(out.status[n > 64] == ref.TOO_MANY_EDGES)
    assert len(out.faces) == len(faces) + (n[n <= 64] - 2).sum()
    assert cases.euler(out.faces) == cases.euler(faces) + (n <= 64).sum()
    before, after = cases.border_count(faces, len(verts)), cases.border_count(out.faces, len(verts))
    assert after == (before[0] - n[n <= 64].sum(), 0)
    # between two perimeters only the smaller hole closes
    per = out.perimeter
    a, b = np.argsort(per)[:2]
    mid = 0.5 * (per[a] + per[b])
    st = ref.close_holes(verts, faces, max_edges=64, max_perimeter=mid).status
    assert st[a] == ref.FILLED and np.all(np.delete(st, a) != ref.FILLED) and st[b] == ref.PERIMETER


def test_refusal_of_a_patch_that_would_duplicate():
    verts, faces = cases.strip_over_hole()
    out = ref.close_holes(verts, faces)
    n = np.diff(out.loops.loop_off)
    assert sorted(n.tolist()) == [3, 3, 4, 20]
    assert np.all(out.status[n <= 4] == ref.DUPLICATE)
    assert len(out.faces) == len(faces) + (n - 2)[out.status == ref.FILLED].sum()
    assert not np.any(np.isin(out.new_face_loop, np.nonzero(n <= 4)[0]))


def test_two_patches_never_share_an_edge():
    verts, faces = cases.shared_diagonal()
    out = ref.close_holes(verts, faces)
    lp = out.loops
    assert np.diff(lp.loop_off).tolist() == [4, 4, 4, 4] and lp.closed.all()
    inner = [l for l in range(4) if {0, 2} <= set(lp.loop_vertex[lp.loop_off[l]:lp.loop_off[l + 1]].tolist())]
    assert len(inner) == 2
    assert out.status[inner[0]] == ref.FILLED and out.status[inner[1]] == ref.DUPLICATE
    new = out.faces[len(faces):][out.new_face_loop == inner[0]]
    assert all({0, 2} <= set(t.tolist()) for t in new)          # the first patch is split along p-q
    assert not np.any(out.new_face_loop == inner[1])
    assert cases.border_count(out.faces, len(verts)) == (4, 0)  # the refused rim stays border, no edge has three faces


def test_saddle_is_not_a_fan():
    verts, faces = cases.annulus(12, saddle=0.8)
    out = ref.close_holes(verts, faces)
    new = out.faces[len(faces):]
    inner = new[np.all(new < 12, 1)]                            # the patch of the saddle-shaped inner loop
    assert len(inner) == 10
    apex = np.bincount(inner.reshape(-1), minlength=12)
    assert apex.max() < 10                                      # a fan has one vertex in all ten triangles
