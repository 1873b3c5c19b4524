"""CPU: the numpy restatement of the remeshing kernels (tests/meshremesh_ref.py) held to what it was not built from: after
every sub-round the winners are independent, the surface keeps its topology (Euler characteristic, half-edges per edge,
no duplicate or degenerate face, the winding), a flip round lowers the valence deviation by exactly its gains, a collapse
round leaves no long edge at a kept vertex, the border keeps its edges where it must -- and the edge lengths gather
around the target."""
import numpy as np
import pytest

import meshremesh_ref as R
import meshsubdiv_ref as S

NAMES = ("ico0", "fan", "three", "awkward", "sheet", "stretched", "cube", "sphere", "squashed_ico2")
FACTORS = (0.5, 1.0, 1.5)
MESHES = R.meshes()
WOUND = ("ico0", "squashed_ico2")


def _closed(T, w):
    return set(R.ring_of(T, w).tolist()) | {int(w)}


def _no_repeats(faces):
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    triples = np.sort(faces, 1)
    assert len(np.unique(triples, axis=0)) == len(triples)


def _proper(faces):
    """the faces without a repeated vertex (the awkward mesh brings three of its own, which no step touches)"""
    return faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]


def _faces_at(faces, mask):
    """the faces with a corner in `mask`, as sorted triples"""
    return {tuple(sorted(t)) for t in faces[mask[faces].any(1)].tolist()}


def _chi(pos, faces):
    v, e, f, hist = S.euler(pos, faces)
    return v - e + f, hist


class _Watch:
    """checks every sub-round of a run as the driver reports it"""

    def __init__(self, name, high, border_angle):
        self.name, self.high, self.border_angle = name, high, border_angle
        self.rounds = dict(split=0, collapse=0, flip=0, relax=0)
        self.winners = dict(collapse=0, flip=0)

    def __call__(self, kind, pos, faces, **kw):
        self.rounds[kind] += 1
        if kind in ("collapse", "flip"):
            getattr(self, kind)(pos, faces, **kw)
        if self.name in WOUND:
            out = kw.get("faces_out", faces)
            assert R.consistently_wound(out, len(pos)), kind

    def collapse(self, pos, faces, T, status, keep, gone, rank, win, pos_out, faces_out):
        t = T.table
        e = np.nonzero(win)[0]
        self.winners["collapse"] += len(e)
        assert len(e) >= 1 and (status[e] == R.CANDIDATE).all()        # the candidate of the smallest rank always wins
        seen = set()
        for i in e:                                                      # N[u] + N[v] of the winners: pairwise disjoint
            mine = _closed(T, t.u[i]) | _closed(T, t.v[i])
            assert not (mine & seen), "two collapses share a vertex of their neighbourhoods"
            seen |= mine
            assert {int(keep[i]), int(gone[i])} == {int(t.u[i]), int(t.v[i])} and T.vclass[gone[i]] < 2
        chi0, hist0 = _chi(pos, faces)
        chi1, hist1 = _chi(pos_out, faces_out)
        assert chi1 == chi0
        assert {c: n for c, n in hist0.items() if c >= 3} == {c: n for c, n in hist1.items() if c >= 3}
        assert hist1.get(1, 0) <= hist0.get(1, 0) and hist1.get(2, 0) <= hist0.get(2, 0)
        assert hist1.get(1, 0) + hist1.get(2, 0) < hist0.get(1, 0) + hist0.get(2, 0)
        _no_repeats(_proper(faces_out))
        assert len(faces_out) - len(_proper(faces_out)) == len(faces) - len(_proper(faces))
        stay = T.vclass == 2
        np.testing.assert_array_equal(pos_out[stay], pos[stay])
        assert not stay[gone[e]].any() and _faces_at(faces, stay) <= _faces_at(faces_out, stay)
        moved = np.nonzero((pos_out != pos).any(1))[0]
        assert set(moved.tolist()) <= set(keep[e].tolist())
        after = R.topo(faces_out, len(pos))
        for k in keep[e]:                                                # no edge at a kept vertex exceeds high
            ring = R.ring_of(after, k)
            if len(ring):
                assert R._dist2(pos_out[ring], pos_out[k]).max() <= self.high * self.high
        if self.border_angle == 0.0:
            assert R.border_edges(faces_out, len(pos)) == R.border_edges(faces, len(pos))

    def flip(self, pos, faces, T, status, gain, ab, rank, win, faces_out):
        t = T.table
        e = np.nonzero(win)[0]
        self.winners["flip"] += len(e)
        assert len(e) >= 1 and (status[e] == R.CANDIDATE).all() and (gain[e] > 0).all()
        quads = np.stack([t.u[e], t.v[e], ab[e, 0], ab[e, 1]], 1)
        assert len(np.unique(quads)) == quads.size, "two flips share a vertex"
        assert _chi(pos, faces_out) == _chi(pos, faces)
        _no_repeats(_proper(faces_out))
        assert len(faces_out) == len(faces) and (faces_out != faces).any(1).sum() == 2 * len(e)
        after = R.topo(faces_out, len(pos))

        def deviation(X):
            return int(((R.valence(X) - R.target_valence(X)) ** 2).sum())
        np.testing.assert_array_equal(after.vclass, T.vclass)
        assert _faces_at(faces, T.vclass == 2) == _faces_at(faces_out, T.vclass == 2)
        assert deviation(T) - deviation(after) == int(gain[e].sum())
        assert R.border_edges(faces_out, len(pos)) == R.border_edges(faces, len(pos))
        new = {(min(a, b), max(a, b)) for a, b in ab[e].tolist()}       # the new edges are there, the old ones gone
        have = set(zip(after.table.u.tolist(), after.table.v.tolist()))
        assert new <= have and not ({(int(t.u[i]), int(t.v[i])) for i in e} & have)


@pytest.fixture(scope="module")
def runs():
    """the restatement's driver, watched, once per mesh and target length (two iterations, without the projection)"""
    out = {}
    for name in NAMES:
        v, f = MESHES[name]
        mean = R.mean_edge(v, f)
        for factor in FACTORS:
            target = factor * mean
            watch = _Watch(name, target * 4 / 3, 30.0)
            out[name, factor] = (R.remesh_isotropic(v, f, target, iterations=2, project=False, trace=watch), watch)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_sub_round_keeps_the_surface(name, runs):
    v, f = MESHES[name]
    for factor in FACTORS:
        got, watch = runs[name, factor]
        assert watch.rounds["split"] == 2 and got.iterations == 2
        assert len(got.collapsed) == len(got.flipped) == len(got.split) == 2
        assert sum(got.collapsed) == watch.winners["collapse"] and sum(got.flipped) == watch.winners["flip"]
        assert np.isfinite(got.verts).all() and got.faces.min() >= 0 and got.faces.max() < len(got.verts)
        assert len(np.unique(got.faces)) == len(got.verts)               # compacted: every vertex is used
        _no_repeats(_proper(got.faces))
        if name != "awkward":                        # (a split of its faces with a repeated vertex adds self-edges)
            assert _chi(got.verts, got.faces)[0] == _chi(v, f)[0]


def test_something_happens_on_every_path(runs):
    """the watched runs reach splits, collapses of edges with two faces and with one, and flips"""
    assert sum(sum(r.split) for r, _ in runs.values()) > 0
    assert sum(w.winners["collapse"] for _, w in runs.values()) > 100
    assert sum(w.winners["flip"] for _, w in runs.values()) > 100
    assert sum(runs["sheet", 1.5][0].collapsed) > 0 and sum(runs["stretched", 0.5][0].split) > 0
    v, f = MESHES["sheet"]
    assert R.border_edges(runs["sheet", 1.5][0].faces, len(runs["sheet", 1.5][0].verts)) < R.border_edges(f, len(v))


@pytest.mark.parametrize("name", ["sheet", "fan", "stretched", "awkward"])
def test_a_border_angle_of_zero_keeps_every_border_edge_in_the_collapses(name):
    v, f = MESHES[name]
    target = 1.5 * R.mean_edge(v, f)
    watch = _Watch(name, target * 4 / 3, 0.0)
    got = R.remesh_isotropic(v, f, target, iterations=2, project=False, border_angle=0.0, trace=watch)
    assert watch.rounds["collapse"] >= 1 or sum(got.collapsed) == 0


def test_an_icosahedron_at_its_own_edge_length_stays():
    v, f = MESHES["ico0"]
    target = R.mean_edge(v, f)
    got = R.remesh_isotropic(v, f, target, iterations=3, project=False)
    assert got.split == got.collapsed == got.flipped == (0, 0, 0)
    np.testing.assert_array_equal(got.faces, f)
    np.testing.assert_allclose(got.verts, v, atol=1e-15)               # relaxed about its own ring's mean: where it was


@pytest.mark.parametrize("name", ["three", "awkward"])
def test_vertices_that_stay_keep_their_place(name, runs):
    """(their faces: checked round by round above; a split may cut them, no collapse or flip touches them)"""
    v, f = MESHES[name]
    stay = np.nonzero(R.topo(f, len(v)).vclass == 2)[0]
    assert len(stay)
    for factor in FACTORS:
        got = runs[name, factor][0]
        have = set(map(tuple, got.verts.tolist()))
        assert all(tuple(p) in have for p in v[stay].tolist()), factor
    if name == "three":                              # every edge has an end that stays: only splits
        assert all(sum(runs[name, k][0].collapsed) == sum(runs[name, k][0].flipped) == 0 for k in FACTORS)
        np.testing.assert_array_equal(runs[name, 1.5][0].faces, f)


@pytest.mark.parametrize("name,target", [("squashed_ico2", 0.25), ("sphere", None)])
def test_the_edges_gather_around_the_target(name, target):
    v, f = MESHES[name]
    target = 1.5 * R.mean_edge(v, f) if target is None else target
    got = R.remesh_isotropic(v, f, target, iterations=3, project=False)
    before, after = R.quality(v, f, target), R.quality(got.verts, got.faces, target)
    for label, q, n in (("input ", before, len(f)), ("output", after, len(got.faces))):
        print(f"{name} at L = {target:.4g}, {label}: {n} faces, share of edges in [0.8 L, 4/3 L] {q[0]:.3f}, "
              f"triangle quality min {q[1]:.3f} mean {q[2]:.3f}, edge length spread {q[3]:.3f}")
    print(f"{name}: split {got.split}, collapsed {got.collapsed}, flipped {got.flipped}")
    assert after[0] > before[0]


def test_the_statuses_name_every_reason():
    """each code of the header is met on the nine meshes, a sheet jittered in its plane, a dented disk and a
    tetrahedron"""
    seen_c, seen_f = set(), set()
    for v, f in list(MESHES.values()) + [R.jittered_sheet(), R.dented_disk(), R.tetrahedron()]:
        T = R.topo(f, len(v))
        mean = R.mean_edge(v, f)
        for high in (1.6, 3.0):
            seen_c |= set(R.collapse_check(v, f, T, 1.2 * mean, high * mean, np.cos(np.radians(30.0)))[0].tolist())
        seen_f |= set(R.flip_check(v, f, T)[0].tolist())
    assert seen_c == {R.CANDIDATE, R.COUNT, R.LONG, R.CLASS, R.BORDER, R.LINK, R.REACH, R.FOLD, R.DUPLICATE}
    assert seen_f == {R.CANDIDATE, R.COUNT, R.CLASS, R.SAME, R.EXISTS, R.GAIN, R.FOLD}
