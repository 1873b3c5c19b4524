"""GPU: generalised winding numbers (neuraludf_amd/evaluation.py MeshIndex.winding / winding_number / contains_points and
signed_distance with method="winding", csrc/meshwinding.hip) against the numpy restatement (tests/meshwinding_ref.py): the
tree and the node records bit for bit, per query the number of faces evaluated exactly and of nodes replaced by their
expansion, and the value within a bound derived from the terms summed; independence of a query from its wave mates, of
the run and of the leaf size; the reason for the feature (a sphere with holes) and the CLI word.  The restatement of an
input is computed once.

The bound: n terms are summed, each re-rounded once per later addition.  Everything but atan2 is bit-equal; atan2 is taken
to be within 1e-15 of numpy's as in test_gpu_meshorient.py, i.e. <= 1.6e-16 per term after / 4 pi, and the re-rounded
partial sums add <= 1.1e-16 sum|term| / 4 pi per term; the bar is n 1e-15 max(1, sum|term| / 4 pi), three times their sum."""
import functools
import math

import numpy as np
import pytest
import torch

import meshray_ref
import meshwinding_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BETAS = (1.0, 2.0, 3.0, math.inf)
MESHES = ("sphere", "sheets", "moebius", "fan", "punched", "absent")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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
    if name == "punched":
        return R.punched_sphere()
    if name == "absent":
        return R.with_absent_faces(*meshray_ref.icosphere(2))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _queries(name):
    """random points in the grown box, then: far outside the box (the root itself is far), a vertex, a point on a face,
    a point in a face's plane outside the face; 65 + 8 points, about 2 000 for the punched sphere"""
    v, f = _mesh(name)
    fin = v[np.isfinite(v).all(1)]
    lo, hi = fin.min(0), fin.max(0)
    ext = (hi - lo).max()
    rng = np.random.default_rng(7)
    n = 1500 if name == "punched" else 57
    q = [rng.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (n, 3))]
    if name == "punched":
        q.append(R.shell_points(2, 0.6, (0.5, 0.8, 1.25)))
    centre = 0.5 * (lo + hi)
    q.append(centre + 40.0 * ext * np.array([[1.0, 0.2, -0.3], [-0.5, 1.0, 0.1], [0.1, -0.2, -1.0], [1.0, 1.0, 1.0]]))
    face = f[len(f) // 2]
    p0, p1, p2 = v[face]
    q.append(np.stack([p0, (p0 + (p1 + p2)) / 3.0, 0.5 * (p0 + p1), p0 + 2.0 * (p1 - p0)]))
    q.append(rng.uniform(lo, hi, (8, 3)))
    return np.concatenate(q)


@functools.lru_cache(maxsize=None)
def _index(name, factor=None):
    """(the MeshIndex with its tree built, the restatement's tree at the same leaf edge); read only"""
    from neuraludf_amd import evaluation as E
    v, f = _mesh(name)
    idx = E.MeshIndex(_dev(v), _dev(f))
    old = E.WINDING_LEAF_FACTOR
    try:
        if factor is not None:
            E.WINDING_LEAF_FACTOR = factor
        idx.winding(_dev(_queries(name)[:1]))
    finally:
        E.WINDING_LEAF_FACTOR = old
    leaf = idx._winding_tree.leaf
    want = R.leaf_grid(np.array(idx.lo), np.array(idx.hi), R.default_leaf(v, f, factor))[0]
    assert abs(leaf / want - 1.0) < 1e-12                                   # torch's mean against numpy's
    return idx, R.Tree(v, f, leaf=leaf)


@functools.lru_cache(maxsize=None)
def _want(name, beta, factor=None):
    return R.winding(_index(name, factor)[1], _queries(name), beta)


def _run(idx, q, beta):
    w, exact, far = idx.winding(q if isinstance(q, torch.Tensor) else _dev(q), beta, _counts=True)
    assert w.dtype == torch.float64 and exact.dtype == torch.int64 and far.dtype == torch.int64
    return w.cpu().numpy(), exact.cpu().numpy(), far.cpu().numpy()


def _check(got, want, rows=slice(None)):
    w, exact, far = got
    assert np.array_equal(exact, want["exact"][rows]) and np.array_equal(far, want["far"][rows])
    n = want["exact"][rows] + want["far"][rows]
    bar = n * 1e-15 * np.maximum(1.0, want["abs"][rows])
    err = np.abs(w - want["w"][rows])
    assert (err <= bar).all(), (err.max(), (err / np.maximum(bar, 1e-300)).max())
    only_far = want["exact"][rows] == 0
    assert w[only_far].tobytes() == want["w"][rows][only_far].tobytes()
    return only_far


@pytest.mark.parametrize("name", MESHES)
def test_tree_and_node_records_equal_the_restatement_bit_for_bit(name):
    idx, ref = _index(name)
    t = idx._winding_tree
    assert t.n_nodes == ref.n_nodes and t.grid == ref.grid
    assert np.array_equal(t.faces.cpu().numpy(), ref.sorted_faces)
    assert np.array_equal(t.first.cpu().numpy(), ref.first) and np.array_equal(t.count.cpu().numpy(), ref.end - ref.first)
    assert np.array_equal(t.skip.cpu().numpy(), ref.skip) and np.array_equal(t.level.cpu().numpy(), ref.level)
    assert t.rec.shape == (ref.n_nodes, 32) and t.rec.cpu().numpy().tobytes() == ref.rec.tobytes()
    if name == "fan":
        assert (ref.end - ref.first)[ref.is_leaf].max() > 64                # the hub's leaf
    if name == "punched":
        assert ref.level.max() + 1 >= 4
    if name == "absent":
        assert len(ref.sorted_faces) == len(_mesh(name)[1]) - 3 and ref.sorted_faces.min() == 3


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("name", MESHES)
def test_counts_equal_and_values_within_the_derived_bound(name, beta):
    idx, ref = _index(name)
    q = _queries(name)
    want = _want(name, beta)
    only_far = _check(_run(idx, q, beta), want)
    if beta == math.inf:
        assert (want["far"] == 0).all() and (want["exact"] == len(ref.sorted_faces)).all()
    elif beta == 2.0:
        assert only_far.sum() >= 4 and (want["far"][-16:-12] == 1).all()   # far outside: the root is one expansion
    if name == "sphere":                                                     # 1, 63 and 65 queries: less and more than a wave
        for n in (1, 63, 65):
            _check(_run(idx, q[:n], beta), want, slice(0, n))


def test_points_in_a_faces_plane_get_nothing_from_that_face():
    """one triangle: a vertex, a point on the face, on an edge, in the plane outside: exactly 0; above: an eighth"""
    from neuraludf_amd import evaluation as E
    v = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    q = np.array([[1.0, 0, 0], [0.25, 0.25, 0.5], [0.5, 0.5, 0.0], [2.0, -1.0, 0.0], [0.0, 0.0, 0.0]])
    w = E.winding_number(_dev(q), (_dev(v), _dev(np.array([[0, 1, 2]]))), beta=math.inf).cpu().numpy()
    ref = R.winding(R.Tree(v, np.array([[0, 1, 2]])), q, math.inf)["w"]
    assert (w[:4] == 0).all() and abs(abs(w[4]) - 0.125) < 1e-15 and np.abs(w - ref).max() <= 1e-15


@pytest.mark.parametrize("name", ["punched", "fan"])
def test_a_query_does_not_depend_on_its_wave_mates_or_the_run(name):
    idx, _ = _index(name)
    q = _queries(name)
    for beta in (2.0, math.inf):
        base = _run(idx, q, beta)
        again = _run(idx, q, beta)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
        perm = np.random.default_rng(3).permutation(len(q))
        for order in (np.arange(len(q))[::-1].copy(), perm):
            got = _run(idx, q[order], beta)
            assert all(a.tobytes() == b[order].tobytes() for a, b in zip(got, base))
        for k in (0, 5, len(q) - 14, len(q) - 11, len(q) - 3):               # alone in their wave
            got = _run(idx, q[k:k + 1], beta)
            assert all(a.tobytes() == b[k:k + 1].tobytes() for a, b in zip(got, base))


@pytest.mark.parametrize("factor", [0.5, 4.0])
def test_every_leaf_size_matches_its_own_restatement_and_decides_the_same(factor):
    from neuraludf_amd import evaluation as E
    name = "punched"
    idx, ref = _index(name, factor)
    base, base_ref = _index(name)
    assert ref.n_nodes != base_ref.n_nodes and idx._winding_tree.rec.cpu().numpy().tobytes() == ref.rec.tobytes()
    q = _queries(name)
    for beta in (2.0, math.inf):
        _check(_run(idx, q, beta), _want(name, beta, factor))
    # the decision |w| > 0.5 of the containment fixture is the same at every leaf size
    pts = R.shell_points(2, 0.6, (0.5, 0.8, 1.25))
    a, b = idx.winding(_dev(pts)).abs() > 0.5, base.winding(_dev(pts)).abs() > 0.5
    assert torch.equal(a, b) and E.WINDING_LEAF_FACTOR == R.WINDING_LEAF_FACTOR


def test_float32_input():
    from neuraludf_amd import evaluation as E
    v, f = _mesh("moebius")
    q = _queries("moebius")
    v32, q32 = v.astype(np.float32), q.astype(np.float32)
    idx = E.MeshIndex(_dev(v32), _dev(f.astype(np.int32)))
    got = _run(idx, _dev(q32), 2.0)
    ref = R.Tree(v32.astype(np.float64), f, leaf=idx._winding_tree.leaf)
    _check(got, R.winding(ref, q32.astype(np.float64), 2.0))


def test_inside_by_winding_equals_parity_on_a_closed_sphere_and_beats_it_on_a_punched_one():
    from neuraludf_amd import evaluation as E
    idx, _ = _index("sphere")
    pts = R.shell_points(2, 1.0, (0.5, 0.8, 1.25))
    inside = np.r_[np.ones(324, bool), np.zeros(162, bool)]
    parity = E.contains_points(_dev(pts), idx)
    assert torch.equal(parity, E.contains_points(_dev(pts), idx, method="parity"))
    assert np.array_equal(parity.cpu().numpy(), inside)
    assert torch.equal(E.contains_points(_dev(pts), idx, method="winding"), parity)
    v, f = _mesh("sphere")
    flipped = (_dev(v), _dev(f[:, [0, 2, 1]]))                               # wound inward as a whole
    assert torch.equal(E.contains_points(_dev(pts), flipped, method="winding"), parity)
    assert E.winding_number(_dev(pts[:4]), flipped).max() < -0.99
    sd_p, sd_w = E.signed_distance(_dev(pts), idx), E.signed_distance(_dev(pts), idx, method="winding")
    assert sd_p.cpu().numpy().tobytes() == sd_w.cpu().numpy().tobytes() and (sd_w.cpu().numpy() < 0).sum() == 324
    # the punched sphere of tests/test_meshwinding_ref.py: a ray leaves through a hole, the winding number does not care
    pidx, _ = _index("punched")
    pts = R.shell_points(2, 0.6, (0.5, 0.8, 1.25))
    parity = E.contains_points(_dev(pts), pidx).cpu().numpy()
    winding = E.contains_points(_dev(pts), pidx, method="winding").cpu().numpy()
    assert (parity != inside).sum() >= 1 and np.array_equal(winding, inside)
    assert ((E.signed_distance(_dev(pts), pidx, method="winding").cpu().numpy() < 0) == inside).all()
    for bad in ("rays", None, 1):
        with pytest.raises(ValueError):
            E.contains_points(_dev(pts), idx, method=bad)
        with pytest.raises(ValueError):
            E.signed_distance(_dev(pts), idx, method=bad)


def test_arguments_and_empty_input():
    from neuraludf_amd import evaluation as E
    idx, _ = _index("sphere")
    assert idx.winding(torch.zeros((0, 3), device=DEV)).shape == (0,)
    assert all(x.shape == (0,) for x in idx.winding(torch.zeros((0, 3), device=DEV), _counts=True))
    for bad in ([[math.nan, 0.0, 0.0]], [[0.0, math.inf, 0.0]]):
        with pytest.raises(ValueError):
            idx.winding(torch.tensor(bad, dtype=torch.float64, device=DEV))
    for beta in (0.5, math.nan, -2.0):
        with pytest.raises(ValueError):
            idx.winding(_dev(_queries("sphere")), beta)
    with pytest.raises(ValueError):
        E.winding_number(_dev(_queries("sphere")), "mesh")
    # a mesh without a face that has an area: nothing winds around anything
    flat = E.MeshIndex(_dev(np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])), _dev(np.array([[0, 1, 2]])))
    w, exact, far = flat.winding(_dev(_queries("sphere")), _counts=True)
    assert (w == 0).all() and (exact == 0).all() and (far == 0).all()
    events = {}
    v, f = _mesh("sphere")
    fresh = E.MeshIndex(_dev(v), _dev(f))
    fresh.winding(_dev(_queries("sphere")), _events=events)
    assert list(events) == ["keys", "sort", "levels", "moments", "query_sort", "winding"]
    events = {}
    fresh.winding(_dev(_queries("sphere")), _events=events)                  # the tree is kept
    assert list(events) == ["query_sort", "winding"]


def test_cli_word(tmp_path, capsys):
    from neuraludf_amd import evaluation as E, meshing
    v, f = _mesh("sphere")
    v32 = v.astype(np.float32)                                              # a PLY file stores float32
    q32 = _queries("sphere").astype(np.float32)
    meshing.write_ply(tmp_path / "m.ply", v32, f)
    meshing.write_points_ply(tmp_path / "p.ply", q32, np.zeros((len(q32), 3), np.uint8))
    out = tmp_path / "w.npy"
    assert E.main(["winding", "--mesh", str(tmp_path / "m.ply"), "--points", str(tmp_path / "p.ply"), "--out", str(out),
                   "--beta", "3"]) == 0
    idx = E.MeshIndex(_dev(v32), _dev(f))
    want = idx.winding(_dev(q32), 3.0).cpu().numpy()
    got = np.load(out)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert f"points: {len(q32)}; inside (|w| > 0.5): {int((np.abs(want) > 0.5).sum())};" in capsys.readouterr().out
    # a grid over the box; a mesh with a third of its faces turned round, put right by --orient
    turned = f.copy()
    turned[::3] = turned[::3][:, [0, 2, 1]]
    meshing.write_ply(tmp_path / "t.ply", v32, turned)
    assert E.main(["winding", "--mesh", str(tmp_path / "t.ply"), "--grid", "5", "--out", str(out), "--orient"]) == 0
    grid = np.load(out)
    axes = [torch.linspace(l, h, 5, dtype=torch.float64) for l, h in zip(idx.lo, idx.hi)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    assert grid.shape == (5, 5, 5) and grid.tobytes() == idx.winding(pts).cpu().numpy().tobytes()
    assert grid[2, 2, 2] > 0.99 and abs(grid[0, 0, 0]) < 0.01
    assert E.main(["winding", "--mesh", str(tmp_path / "t.ply"), "--grid", "5", "--out", str(out)]) == 0
    assert np.abs(np.load(out)[2, 2, 2] - 1.0 / 3.0) < 0.05                 # without it a third of the sky cancels twice
    with pytest.raises(SystemExit):
        E.main(["winding", "--mesh", str(tmp_path / "m.ply"), "--out", str(out)])
