"""CPU: the numpy restatement of the Chamfer evaluation (tests/pointcloud_ref.py) against sklearn's KD-tree engine, the
PLY reader / writer, load_dtu_obs, the CPU-side parts of neuraludf_amd/evaluation.py (DTU selection, plane, colours, log
format) against the restatement, and the argument checks that run before any GPU work."""
import math

import numpy as np
import pytest
import torch

import pointcloud_ref as R
from neuraludf_amd import evaluation as E
from neuraludf_amd import meshing


def _clouds(seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 3, (1500, 3))
    d = rng.normal(size=(1500, 3))
    s = d / np.linalg.norm(d, axis=1, keepdims=True) + rng.normal(scale=0.01, size=(1500, 3))
    return np.concatenate([u, s, s[:100]])[rng.permutation(3100)]


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_thinning_equals_sklearn_loop(seed):
    skln = pytest.importorskip("sklearn.neighbors")
    p = _clouds(seed)
    r = 0.1
    eng = skln.NearestNeighbors(n_neighbors=1, radius=r, algorithm="kd_tree").fit(p)
    nbrs = eng.radius_neighbors(p, radius=r, return_distance=False)
    mask = np.ones(len(p), dtype=np.bool_)
    for cur, idx in enumerate(nbrs):
        if mask[cur]:
            mask[idx] = 0
            mask[cur] = 1
    mine = R.radius_neighbors(p, r)
    assert all(np.array_equal(np.sort(a), b) for a, b in zip(nbrs, mine))
    np.testing.assert_array_equal(R.thin(p, r), mask)


def test_restatement_thinning_lattice_ties():
    skln = pytest.importorskip("sklearn.neighbors")
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    nbrs = skln.NearestNeighbors(radius=1.0, algorithm="kd_tree").fit(g).radius_neighbors(g, return_distance=False)
    assert all(np.array_equal(np.sort(a), b) for a, b in zip(nbrs, R.radius_neighbors(g, 1.0)))
    assert len(R.radius_neighbors(g, 1.0)[0]) == 4                # itself and three at exactly 1


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_nearest_equals_sklearn(seed):
    skln = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(seed + 10)
    ref = _clouds(seed)
    q = np.concatenate([rng.uniform(-1, 4, (800, 3)), ref[:50]])
    dist, idx = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(ref).kneighbors(q, n_neighbors=1)
    d, i = R.nearest(q, ref)
    np.testing.assert_array_equal(d, dist[:, 0])
    assert (i == idx[:, 0]).mean() > 0.99                        # ties aside, the same point
    assert (d[800:] == 0).all()
    db, ib = R.nearest(q, ref, bound=0.05)
    far = d > 0.05
    assert (db[far] == np.inf).all() and (ib[far] == -1).all() and (db[~far] == d[~far]).all()


def test_restatement_sampling_counts():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=np.float64)
    p = R.sample_mesh(v, np.array([[0, 1, 2], [3, 3, 0]]), 0.25)
    # thr = 0.25 sqrt(1 / 1), n1 = n2 = 4: (i + .5) / 4 + (j + .5) / 4 < 1  <=>  i + j < 3: 6 points
    assert p.shape == (4 + 6, 3)
    np.testing.assert_array_equal(p[4], [0.125, 0.125, 0.0])


# ---- PLY files ---------------------------------------------------------------------------------------------------------
def test_read_ply_round_trips_write_ply(tmp_path):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(50, 3)).astype(np.float32)
    f = rng.integers(0, 50, (70, 3))
    meshing.write_ply(str(tmp_path / "m.ply"), v, f)
    rv, rf = meshing.read_ply(str(tmp_path / "m.ply"))
    assert rv.dtype == np.float64 and rf.dtype == np.int64
    np.testing.assert_array_equal(rv, v.astype(np.float64))
    np.testing.assert_array_equal(rf, f)
    c = rng.uniform(size=(50, 3))
    meshing.write_points_ply(str(tmp_path / "p.ply"), v.astype(np.float64), c)
    pv, pf = meshing.read_ply(str(tmp_path / "p.ply"))
    assert pf is None
    np.testing.assert_array_equal(pv, v.astype(np.float64))


def test_read_ply_ascii(tmp_path):
    text = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
            "0 0 0 255\n1 0 0 0\n0 1.5 0 3\n0 0 -2e-3 7\n3 0 1 2\n3 0 2 3\n")
    (tmp_path / "a.ply").write_text(text)
    v, f = meshing.read_ply(str(tmp_path / "a.ply"))
    np.testing.assert_array_equal(v, [[0, 0, 0], [1, 0, 0], [0, 1.5, 0], [0, 0, -2e-3]])
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3]])


def test_read_ply_big_endian_extra_properties(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(20, 3))
    f = rng.integers(0, 20, (9, 3))
    vert = np.empty(20, dtype=[("nx", ">f4"), ("x", ">f8"), ("y", ">f8"), ("z", ">f8"), ("red", "u1"), ("green", "u1"),
                               ("blue", "u1"), ("q", ">i2")])
    vert["x"], vert["y"], vert["z"] = v.T
    vert["nx"], vert["red"], vert["q"] = 1.0, 200, -5
    face = np.empty(9, dtype=[("n", "u1"), ("i", ">u4", (3,)), ("flag", "u1")])
    face["n"], face["i"], face["flag"] = 3, f, 1
    head = ("ply\nformat binary_big_endian 1.0\nelement vertex 20\nproperty float nx\nproperty double x\n"
            "property double y\nproperty double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property short q\nelement face 9\nproperty list uint8 uint vertex_indices\nproperty uchar flag\n"
            "element extra 2\nproperty int w\nend_header\n")
    (tmp_path / "b.ply").write_bytes(head.encode() + vert.tobytes() + face.tobytes() + np.zeros(2, ">i4").tobytes())
    rv, rf = meshing.read_ply(str(tmp_path / "b.ply"))
    np.testing.assert_array_equal(rv, v)
    np.testing.assert_array_equal(rf, f)
    # little endian, int32 list, vertex_index name
    face2 = np.empty(9, dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face2["n"], face2["i"] = 3, f
    vl = v.astype("<f4")
    head2 = ("ply\nformat binary_little_endian 1.0\nelement vertex 20\nproperty float x\nproperty float y\n"
             "property float z\nelement face 9\nproperty list uchar int32 vertex_index\nend_header\n")
    (tmp_path / "c.ply").write_bytes(head2.encode() + vl.tobytes() + face2.tobytes())
    rv, rf = meshing.read_ply(str(tmp_path / "c.ply"))
    np.testing.assert_array_equal(rv, vl.astype(np.float64))
    np.testing.assert_array_equal(rf, f)


def test_read_ply_rejects_bad_files(tmp_path):
    (tmp_path / "x.ply").write_bytes(b"not a ply\n")
    with pytest.raises(ValueError):
        meshing.read_ply(str(tmp_path / "x.ply"))
    text = ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 1 1\n3 0 1 5\n")
    (tmp_path / "y.ply").write_text(text)
    with pytest.raises(ValueError, match="out of range"):
        meshing.read_ply(str(tmp_path / "y.ply"))


# ---- DTU files and the CPU-side selection ------------------------------------------------------------------------------
def test_load_dtu_obs(tmp_path):
    sio = pytest.importorskip("scipy.io")
    (tmp_path / "ObsMask").mkdir()
    obs = np.random.default_rng(4).uniform(size=(6, 7, 8)) > 0.5
    bb = np.array([[-10.5, 3.0, 7.25], [40.0, 50.0, 60.0]])
    sio.savemat(str(tmp_path / "ObsMask" / "ObsMask24_10.mat"), dict(ObsMask=obs.astype(np.uint8), BB=bb,
                                                                    Res=np.array([[0.2]])))
    sio.savemat(str(tmp_path / "ObsMask" / "Plane24.mat"), dict(P=np.array([[0.1], [0.2], [0.3], [-4.0]])))
    o, b, r, p = E.load_dtu_obs(str(tmp_path), 24)
    np.testing.assert_array_equal(o, obs)
    np.testing.assert_array_equal(b, bb)
    assert r == 0.2
    np.testing.assert_array_equal(p, [0.1, 0.2, 0.3, -4.0])


def test_dtu_selection_plane_and_colours_on_cpu():
    rng = np.random.default_rng(5)
    obs = rng.uniform(size=(30, 20, 10)) > 0.3
    bb = np.array([[0.1, -3.3, 2.7], [30.2, 17.0, 12.9]])
    down = rng.uniform(-5, 40, (20000, 3))
    down[:100] = np.float32(bb[0]) + 0.5 * rng.integers(-4, 60, (100, 3))      # half-way grid ties (round half to even)
    inbound, rows = E.dtu_masks(torch.as_tensor(down), bb, 0.5, torch.as_tensor(obs), 3.3)
    ri, rr = R.dtu_select(down, bb, 0.5, obs, 3.3)
    np.testing.assert_array_equal(inbound.numpy(), ri)
    np.testing.assert_array_equal(rows.numpy(), rr)
    assert 0 < len(rr) < ri.sum() < len(down)
    plane = np.array([0.31, -0.7, 0.05, 1.3])
    np.testing.assert_array_equal(E.above_plane(torch.as_tensor(down), plane).numpy(), R.above_plane(down, plane))
    d = torch.as_tensor(np.concatenate([rng.uniform(0, 30, len(rr) - 2), [math.inf, 20.0]]))
    np.testing.assert_array_equal(E.vis_colors(d, 10.0, 20.0, len(down), torch.as_tensor(rr)).numpy(),
                                  R.colors(d.numpy(), 10.0, 20.0, len(down), rr))
    np.testing.assert_array_equal(E.vis_colors(d, 10.0, 20.0).numpy(), R.colors(d.numpy(), 10.0, 20.0))
    np.testing.assert_array_equal(E.vis_colors(d, 0.7, 20.0).numpy(), R.colors(d.numpy(), 0.7, 20.0))
    inbound, rows = E.dtu_masks(torch.as_tensor(down), bb, 0.7, torch.as_tensor(obs), 3.3)
    np.testing.assert_array_equal(rows.numpy(), R.dtu_select(down, bb, 0.7, obs, 3.3)[1])


def test_log_format_round_trip():
    res = dict(over_all=1.23456789, mean_d2gt=0.5, mean_gt2d=math.nan, precision_1=0.1234567, recall_1=1.0,
               fscore_1=0.2, precision_2=0.0, recall_2=0.99999, fscore_2=0.5)
    text = E.format_log(res, "scan24", 3)
    assert text.splitlines()[0] == "over_all 1.235 mean_d2gt 0.5 mean_gt2d nan "
    assert text.splitlines()[1] == "precision_1mm 0.123 recall_1mm 1.0 fscore_1mm 0.2 "
    assert text.endswith("[scan24] \n")
    back = E.parse_log(text)
    assert back["stem"] == "scan24" and back["recall_2"] == 1.0 and math.isnan(back["mean_gt2d"])


def test_argument_checks_before_any_gpu_work():
    p = np.zeros((5, 3))
    f = np.array([[0, 1, 2]])
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            E.sample_mesh(p, f, bad)
        with pytest.raises(ValueError):
            E.thin(p, bad)
        with pytest.raises(ValueError):
            E.radius_downsample(p, bad)
        with pytest.raises(ValueError):
            E.chamfer_deepfashion(p, p, max_dist=bad)
        with pytest.raises(ValueError):
            E.chamfer_dtu(p, p, np.ones((2, 2, 2)), np.zeros((2, 3)), 1.0, np.ones(4), downsample_density=bad)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            E.nearest(p, p, bad)
    with pytest.raises(ValueError):
        E.sample_mesh(p[:, :2], f, 0.1)
    with pytest.raises(ValueError):
        E.sample_mesh(p, f.astype(np.float64), 0.1)
    with pytest.raises(ValueError):
        E.sample_mesh(p, f[:, :2], 0.1)
    with pytest.raises(ValueError):
        E.thin(np.zeros((4, 3), dtype=np.int64), 0.1)
    with pytest.raises(ValueError):
        E.nearest(p, p[:0])
    with pytest.raises(ValueError):
        E.chamfer_deepfashion(p, p[:0])
    with pytest.raises(ValueError):
        E.chamfer_dtu(p, p, np.ones((2, 2)), np.zeros((2, 3)), 1.0, np.ones(4))
    with pytest.raises(ValueError):
        E.chamfer_dtu(p, p, np.ones((2, 2, 2)), np.zeros((2, 3)), 0.0, np.ones(4))
    with pytest.raises(ValueError):
        E.chamfer_dtu(p, p, np.ones((2, 2, 2)), np.zeros((2, 3)), 1.0, np.ones(3))
