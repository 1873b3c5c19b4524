"""GPU: the Chamfer evaluation (neuraludf_amd/evaluation.py, csrc/pointcloud.hip) against the numpy restatement
(tests/pointcloud_ref.py) bit for bit -- mesh sampling, thinning, nearest neighbours, the DTU selection -- analytic
distances, both protocols end to end, the CLI and a network end to end.  What it replaces: the reference's
evaluation/eval_dtu_python.py and eval_deepfashion_python.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pointcloud_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _E():
    from neuraludf_amd import evaluation
    return evaluation


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), np.argwhere(a != b)[:5]


# ---- sample_mesh -------------------------------------------------------------------------------------------------------
def _check_sampling(v, f, density):
    got = _np(_E().sample_mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV), density))
    _same(got, R.sample_mesh(v, f, density))
    return len(got)


def test_sample_mesh_random_triangles():
    rng = np.random.default_rng(0)
    v = rng.uniform(-3, 3, (300, 3))
    f = rng.integers(0, 300, (400, 3))
    assert _check_sampling(v, f, 0.3) > 2000


def test_sample_mesh_degenerate_and_special_triangles():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],            # a right triangle
                  [2, 2, 2], [2, 2, 2], [3, 1, 0],            # repeated vertex: zero area
                  [0, 0, 1], [1, 1, 2], [2, 2, 3],            # collinear
                  [np.nan, 0, 0], [0, 5, 0],                  # a NaN vertex
                  [0, 0, 0.001], [0.001, 0, 0.001], [0, 0.001, 0.001],       # tiny (n1 = 0)
                  [0, 0, 5], [100, 0, 5], [0, 0.05, 5]], dtype=np.float64)  # long and skinny
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 1], [0, 9, 2], [11, 12, 13], [14, 15, 16], [2, 1, 0]])
    n = _check_sampling(v, f, 0.05)
    assert n > len(v) + 400


def test_sample_mesh_sphere_mesh():
    """an udf_marching_cubes mesh of an analytic sphere"""
    from neuraludf_amd import meshing
    from neuraludf_amd.models import udf_renderer_blending as rb
    n, box = 48, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    ax = rb._grid_axes(*box, n, DEV)
    X = torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), -1)
    r = X.norm(dim=-1, keepdim=True)
    U, G = (r - 0.6).abs()[..., 0].contiguous(), (X / r * torch.sign(r - 0.6)).contiguous()
    v, f = meshing.udf_marching_cubes(U, G, *box)
    assert f.shape[0] > 1000
    _check_sampling(_np(v).astype(np.float64), _np(f), 0.02)


# ---- thin --------------------------------------------------------------------------------------------------------------
def _check_thin(p, r):
    keep = _np(_E().thin(torch.as_tensor(p, device=DEV), r))
    _same(keep, R.thin(p, r))
    return keep


@pytest.mark.parametrize("seed", [1, 2])
def test_thin_uniform_and_clustered_with_duplicates(seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 4, (3000, 3))
    d = rng.normal(size=(3000, 3))
    s = 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True) + rng.normal(scale=0.01, size=(3000, 3))
    p = np.concatenate([u, s, u[:200], s[:200]])[rng.permutation(6400)]
    keep = _check_thin(p, 0.15)
    assert 0 < keep.sum() < len(p)


def test_thin_lattice_ties_included():
    g = np.stack(np.meshgrid(*[np.arange(12.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = g[np.random.default_rng(3).permutation(len(g))]
    _check_thin(p, 1.0)


def test_thin_sorted_line_long_chain():
    p = np.zeros((1500, 3))
    p[:, 0] = np.arange(1500) * 0.7
    info = {}
    keep = _np(_E().thin(torch.as_tensor(p, device=DEV), 1.0, _info=info))
    _same(keep, R.thin(p, 1.0))
    assert info["rounds"] > 100


def test_thin_tiny_inputs():
    E = _E()
    assert _np(E.thin(torch.zeros((0, 3), dtype=torch.float64, device=DEV), 1.0)).shape == (0,)
    assert _np(E.thin(torch.ones((1, 3), dtype=torch.float64, device=DEV), 1.0)).tolist() == [True]


def test_radius_downsample_seeded():
    E = _E()
    p = torch.as_tensor(np.random.default_rng(4).uniform(0, 1, (4000, 3)), device=DEV)
    a, ia = E.radius_downsample(p, 0.05, seed=0)
    b, ib = E.radius_downsample(p, 0.05, seed=0)
    _same(_np(a), _np(b))
    perm = _np(ia["perm"])
    _same(_np(a), _np(p)[perm][R.thin(_np(p)[perm], 0.05)])
    assert ia["rounds"] >= 1


# ---- nearest -----------------------------------------------------------------------------------------------------------
def _check_nearest(q, r, bound=math.inf, cell=None):
    d, i = _E().nearest(torch.as_tensor(q, device=DEV), torch.as_tensor(r, device=DEV), bound, cell=cell)
    rd, ri = R.nearest(q, r, bound)
    _same(_np(d), rd)
    _same(_np(i), ri)
    return rd


def test_nearest_lattice_faces_and_corners():
    g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    q = np.concatenate([g + 0.5, g[:100] + [0.5, 0, 0], g[:100] + [0.5, 0.5, 0], rng.uniform(-1, 9, (500, 3))])
    for cell in (1.0, 0.5, None):
        _check_nearest(q, g, cell=cell)


def test_nearest_coincident_points_lowest_index():
    r = np.repeat(np.random.default_rng(6).uniform(0, 1, (50, 3)), 4, axis=0)[::-1].copy()
    rd = _check_nearest(r[::3], r)
    assert (rd == 0).all()


def test_nearest_bound_edges():
    r = np.array([[0.0, 0, 0], [10.0, 0, 0]])
    q = np.array([[0, 2.0, 0], [0, 2.0 + 1e-12, 0], [0, 2.0 - 1e-12, 0], [5, 0, 0], [0, 0, 3.0]])
    rd = _check_nearest(q, r, bound=2.0)
    assert rd[0] == 2.0 and rd[1] == math.inf and rd[2] < 2.0 and rd[3] == math.inf
    d, i = _E().nearest(torch.as_tensor(q, device=DEV), torch.as_tensor(r, device=DEV), 2.0)
    assert _np(i)[1] == -1


def test_nearest_bound_stops_the_walk_among_empty_cells():
    """two clusters in opposite corners of a 4 x 4 x 4 grid: a query between them, inside the points' box, walks rings of
    empty cells and stops when the ring's reach passes the bound with nothing met (-1, inf)"""
    rng = np.random.default_rng(9)
    r = np.concatenate([rng.uniform(0.0, 0.3, (6, 3)), rng.uniform(3.6, 3.9, (6, 3))])
    q = np.concatenate([rng.uniform(1.6, 2.4, (30, 3)), rng.uniform(0.0, 0.5, (5, 3)), rng.uniform(3.4, 3.9, (5, 3))])
    rd = _check_nearest(q, r, bound=0.5, cell=1.0)
    assert (rd[:30] == math.inf).all() and (rd[30:] <= 0.5).sum() >= 5
    d, i = _E().nearest(torch.as_tensor(q, device=DEV), torch.as_tensor(r, device=DEV), 0.5, cell=1.0)
    assert (_np(i)[:30] == -1).all()


def test_nearest_far_queries_and_one_point_reference():
    rng = np.random.default_rng(7)
    r = rng.uniform(0, 1, (2000, 3))
    q = rng.uniform(50, 60, (300, 3))
    _check_nearest(q, r)
    _check_nearest(q, r, bound=70.0)
    _check_nearest(q, r, bound=10.0)
    _check_nearest(q, r[:1])
    _check_nearest(rng.uniform(-1, 2, (300, 3)), r[:1])


def test_nearest_empty_reference_raises():
    with pytest.raises(ValueError):
        _E().nearest(torch.zeros((3, 3), dtype=torch.float64, device=DEV),
                     torch.zeros((0, 3), dtype=torch.float64, device=DEV))


def test_nearest_clouds_vs_brute_force():
    rng = np.random.default_rng(8)
    d = rng.normal(size=(20000, 3))
    r = 100.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    q = r[:5000] * rng.uniform(0.9, 1.2, (5000, 1))
    _check_nearest(q, r, bound=20.0)


# ---- analytic case ------------------------------------------------------------------------------------------------------
def test_plane_offset_distances_are_delta():
    """a plane mesh; GT = its own sample points moved by delta along the normal (delta below half the spacing)"""
    E = _E()
    n = 20
    x = np.arange(n + 1, dtype=np.float64)
    v = np.stack(np.meshgrid(x, x, indexing="ij"), -1).reshape(-1, 2)
    v = np.concatenate([v, np.zeros((len(v), 1))], 1)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    delta = 0.15                                      # density 0.5: kept points are more than 0.5 apart
    down, _ = E.radius_downsample(E.sample_mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV), 0.5),
                                  0.5, seed=0)
    gt = _np(down) + np.array([0, 0, delta])
    res = E.chamfer_deepfashion((v, f), gt, downsample_density=0.5, max_dist=1.0, thresholds=(0.1, 0.2))
    d, _ = E.nearest(down, torch.as_tensor(gt, device=DEV))
    assert (_np(d) == delta).all()
    assert abs(res["mean_d2gt"] - delta) < 1e-12 and abs(res["mean_gt2d"] - delta) < 1e-12
    assert res["precision_1"] == 0 and res["recall_1"] == 0 and res["precision_2"] == 1 and res["recall_2"] == 1
    assert res["n_down"] == len(gt)


# ---- the protocols end to end --------------------------------------------------------------------------------------------
def _scan():
    """a wavy sheet in mm, GT on a perturbed copy of it, an ObsMask with holes and a plane cutting part of the GT"""
    rng = np.random.default_rng(9)
    n = 40
    x = np.linspace(0, 80, n + 1)
    X, Y = np.meshgrid(x, x, indexing="ij")
    Z = 10 * np.sin(X / 15) + 5 * np.cos(Y / 11)
    v = np.stack([X, Y, Z], -1).reshape(-1, 3) + [100, 50, 0]
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    gx = rng.uniform(-5, 85, (15000, 2))
    gz = 10 * np.sin(gx[:, 0] / 15) + 5 * np.cos(gx[:, 1] / 11) + rng.normal(scale=0.8, size=15000)
    gt = np.concatenate([gx, gz[:, None]], 1) + [100, 50, 0]
    bb = np.array([[95.0, 45.0, -20.0], [160.0, 110.0, 20.0]])
    res = 2.0
    shape = (50, 50, 25)
    obs = rng.uniform(size=shape) > 0.2
    obs[10:20, 10:25, :] = False
    plane = np.array([0.3, -0.1, 0.05, -20.0])
    return v, f, gt, obs, bb, res, plane


def test_chamfer_dtu_end_to_end():
    E = _E()
    v, f, gt, obs, bb, res, plane = _scan()
    density = 0.5
    out = E.chamfer_dtu((v, f), gt, obs, bb, res, plane, downsample_density=density, patch_size=3.0, seed=3)
    pcd = _np(E.sample_mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV), density))
    _, info = E.radius_downsample(torch.as_tensor(pcd, device=DEV), density, seed=3)
    ref, *_ = R.chamfer_dtu(pcd, _np(info["perm"]), gt, obs, bb, res, plane, density, patch=3.0)
    for k in ("n_data", "n_down", "n_in", "n_in_obs", "n_gt", "n_gt_above"):
        assert out[k] == ref[k], k
    assert 0 < out["n_in_obs"] < out["n_in"] < out["n_down"] and 0 < out["n_gt_above"] < out["n_gt"]
    for k in ("precision_1", "recall_1", "fscore_1", "precision_2", "recall_2", "fscore_2"):
        assert out[k] == ref[k], k
    for k in ("mean_d2gt", "mean_gt2d", "over_all"):
        assert abs(out[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    assert 0 < out["precision_1"] <= out["precision_2"] <= 1 and out["thinning_rounds"] >= 1


def test_dtu_selection_and_colours_match(tmp_path):
    E = _E()
    v, f, gt, obs, bb, res, plane = _scan()
    rng = np.random.default_rng(10)
    down = rng.uniform(85, 200, (20000, 3)) * [1, 1, 0.3]
    inbound, rows = E.dtu_masks(torch.as_tensor(down, device=DEV), bb, res, torch.as_tensor(obs, device=DEV), 7.0)
    ri, rr = R.dtu_select(down, bb, res, obs, 7.0)
    _same(_np(inbound), ri)
    _same(_np(rows), rr)
    _same(_np(E.above_plane(torch.as_tensor(gt, device=DEV), plane)), R.above_plane(gt, plane))
    for r in (0.7, 1.3):                    # resolutions whose reciprocal is inexact
        inbound, rows = E.dtu_masks(torch.as_tensor(down, device=DEV), bb, r, torch.as_tensor(obs, device=DEV), 7.0)
        ri, rr2 = R.dtu_select(down, bb, r, obs, 7.0)
        _same(_np(inbound), ri)
        _same(_np(rows), rr2)
    d = torch.as_tensor(rng.uniform(0, 30, len(rr)), device=DEV)
    for vis in (10.0, 3.0, 0.7):
        _same(_np(E.vis_colors(d, vis, 20.0, len(down), torch.as_tensor(rr, device=DEV))),
              R.colors(_np(d), vis, 20.0, len(down), rr))


def test_chamfer_deepfashion_end_to_end_and_vis(tmp_path):
    E = _E()
    from neuraludf_amd.meshing import read_ply
    v, f, gt, *_ = _scan()
    v, gt = v / 1000.0, gt / 1000.0                         # metres
    out = E.chamfer_deepfashion((v, f), gt, downsample_density=0.0005, seed=1, vis_dir=str(tmp_path), name="007")
    pcd = _np(E.sample_mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV), 0.0005))
    _, info = E.radius_downsample(torch.as_tensor(pcd, device=DEV), 0.0005, seed=1)
    ref, down, d2s, s2d = R.chamfer_deepfashion(pcd, _np(info["perm"]), gt, 0.0005)
    for k in ("n_data", "n_down", "n_gt", "precision_1", "recall_1", "fscore_1", "precision_2", "recall_2", "fscore_2"):
        assert out[k] == ref[k], k
    for k in ("mean_d2gt", "mean_gt2d", "over_all"):
        assert abs(out[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    pv, _ = read_ply(str(tmp_path / "vis_007_d2gt.ply"))
    _same(pv, down)
    gv, _ = read_ply(str(tmp_path / "vis_007_gt2d.ply"))
    _same(gv, gt)


def test_cli_writes_the_reference_log(tmp_path):
    E = _E()
    from neuraludf_amd.meshing import write_ply
    v, f, gt, obs, bb, res, plane = _scan()
    write_ply(str(tmp_path / "mesh.ply"), v, f)
    write_ply(str(tmp_path / "gt.ply"), gt, np.zeros((0, 3), dtype=np.int64))
    v32, gt32 = v.astype(np.float32).astype(np.float64), gt.astype(np.float32).astype(np.float64)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "neuraludf_amd.evaluation"]
    log = tmp_path / "df.txt"
    p = subprocess.run(base + ["deepfashion", "--data", str(tmp_path / "mesh.ply"), "--gt", str(tmp_path / "gt.ply"),
                               "--downsample_density", "0.5", "--max_dist", "20", "--no_vis", "--log", str(log)],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("over_all: ")
    got = E.parse_log(log.read_text())
    want = E.chamfer_deepfashion((v32, f), gt32, downsample_density=0.5, max_dist=20.0)
    text = E.format_log(want, "mesh", 6)
    assert log.read_text() == text and got["stem"] == "mesh"
    for k in ("precision_1", "recall_2", "over_all"):
        assert got[k] == float(np.round(want[k], 6))
    scipy_io = pytest.importorskip("scipy.io")
    os.makedirs(tmp_path / "ObsMask")
    scipy_io.savemat(str(tmp_path / "ObsMask" / "ObsMask5_10.mat"),
                     dict(ObsMask=obs.astype(np.uint8), BB=bb, Res=np.array([[res]])))
    scipy_io.savemat(str(tmp_path / "ObsMask" / "Plane5.mat"), dict(P=plane.reshape(4, 1)))
    p = subprocess.run(base + ["dtu", "--data", str(tmp_path / "mesh.ply"), "--gt", str(tmp_path / "gt.ply"),
                               "--dataset_dir", str(tmp_path), "--scan", "5", "--downsample_density", "0.5",
                               "--patch_size", "3", "--vis_out_dir", str(tmp_path / "vis")],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    want = E.chamfer_dtu((v32, f), gt32, obs, bb, res, plane, downsample_density=0.5, patch_size=3.0)
    assert (tmp_path / "eval_result.txt").read_text() == E.format_log(want, "mesh", 3)
    assert (tmp_path / "vis" / "vis_005_d2gt.ply").exists() and (tmp_path / "vis" / "vis_005_gt2d.ply").exists()


def test_argument_errors():
    E = _E()
    p = torch.rand((10, 3), dtype=torch.float64, device=DEV)
    f = torch.tensor([[0, 1, 2]], device=DEV)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            E.sample_mesh(p, f, bad)
        with pytest.raises(ValueError):
            E.thin(p, bad)
        with pytest.raises(ValueError):
            E.chamfer_deepfashion(p, p, max_dist=bad)
    with pytest.raises(ValueError):
        E.sample_mesh(p, torch.tensor([[0, 1, 10]], device=DEV), 0.1)
    with pytest.raises(ValueError):
        E.sample_mesh(p, torch.tensor([[0, 1, -1]], device=DEV), 0.1)
    with pytest.raises(ValueError, match="max_points"):
        E.sample_mesh(p * 100, torch.tensor([[0, 1, 2], [3, 4, 5]], device=DEV), 1e-4, max_points=10 ** 6)
    q = p.clone()
    q[3, 1] = math.nan
    with pytest.raises(ValueError):
        E.thin(q, 0.1)
    with pytest.raises(ValueError):
        E.nearest(q, p)
    with pytest.raises(ValueError):
        E.chamfer_deepfashion(p, p[:0])
    v, f, gt, obs, bb, res, plane = _scan()
    with pytest.raises(ValueError, match="ObsMask"):
        E.chamfer_dtu(gt + 1000.0, gt, obs, bb, res, plane, downsample_density=1.0)
    with pytest.raises(ValueError, match="plane"):
        E.chamfer_dtu(gt, gt, obs, bb, res, -np.abs(plane) * [0, 0, 0, 1], downsample_density=1.0)


def test_network_end_to_end():
    """UDFNetwork of the shipped DTU conf -> extract_udf_mesh -> chamfer_deepfashion against the mesh's own samples"""
    import contextlib
    import io
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    from neuraludf_amd.train import DTU_MODEL_CONF
    E = _E()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        udf = fields.UDFNetwork(**DTU_MODEL_CONF["udf_network"]).to(DEV)
    v, f = meshing.extract_udf_mesh(udf, 64)
    v = v.astype(np.float64)
    pcd = E.sample_mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV), 0.01)
    gt, _ = E.radius_downsample(pcd, 0.01, seed=0)          # the points the evaluation keeps
    out = E.chamfer_deepfashion((v, f), gt, downsample_density=0.01, max_dist=0.1, thresholds=(0.001, 0.002))
    assert out["mean_d2gt"] == 0.0 and out["mean_gt2d"] == 0.0
    assert out["precision_1"] == 1.0 and out["recall_1"] == 1.0 and out["precision_2"] == 1.0
    assert out["n_data"] == pcd.shape[0] > out["n_down"] == out["n_gt"] > 1000
