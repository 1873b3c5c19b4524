"""GPU: the rasteriser (neuraludf_amd/meshrender.py, csrc/meshraster.hip) against the numpy restatement
(tests/meshraster_ref.py) on the scenes of tests/meshraster_scenes.py: depth, face and barycentrics bit for bit (the
kernels divide with the correctly rounded float64 division, so the barycentrics need no tolerance), the visibility arrays
equal, the colours to one float32 ulp -- plus the two draw paths against each other, determinism, normal_map, the CLI and
the argument checks."""
import functools
import os

import numpy as np
import pytest
import torch

import meshraster_ref as R
import meshraster_scenes as S
from test_meshraster_ply import write_ply_before

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP32 = 2.0 ** -23            # one float32 ulp of 1.0: the colours are float32 casts of float64 values in [0, 1] that differ
#                               from the restatement's by the error of pow alone (~1e-16), so at most a rounding boundary apart


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(raster):
    return tuple(t.cpu().numpy() for t in raster)


def _same(got, want):
    """three buffers bit for bit (+inf depths and -1 faces included)"""
    for g, w, name in zip(got, want, ("depth", "face", "bary")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, int((g != w).sum()))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(verts, faces, mats, H, W, (depth, face, bary), info) of a scene, computed once"""
    if name == "squares":
        (v, f), mats, H, W = S.two_squares(), S.SQ_P, S.SQ_H, S.SQ_W
    elif name == "ragged":
        v, f, mats, _ = S.ragged()
        H, W = S.RAG_H, S.RAG_W
    elif name == "parallel":
        v, f, mats, _ = S.parallel_sheets()
        H, W = S.VIS_H, S.VIS_W
    else:
        v, f = dict(tilt45=lambda: S.tilted_sheet(45.0), tilt80=lambda: S.tilted_sheet(80.0), ridge=S.ridge_sheet)[name]()
        mats, H, W = S.VIS_P, S.VIS_H, S.VIS_W
    info = {}
    return v, f, mats, H, W, R.rasterize(v, f, mats, H, W, info), info


def test_two_square_occlusion_bit_identical():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, want, _ = _ref("squares")
    info = {}
    got = meshrender.rasterize(_dev(v), _dev(f), mats, H, W, _info=info)
    assert isinstance(got, meshrender.Raster) and got.depth.shape == (1, H, W) and got.bary.shape == (1, H, W, 3)
    _same(_np(got), want)
    assert info["skipped"] == 0 and info["small"] + info["large"] == 4
    assert float(got.depth[0, 12, 16]) == 1.0 and float(got.depth[0, 5, 9]) == 2.0 and int(got.face[0, 0, 0]) == -1
    # float32 vertices draw the same picture: the squares' coordinates are exact in float32
    _same(_np(meshrender.rasterize(_dev(v.astype(np.float32)), _dev(f), mats, H, W)), want)


def test_ragged_case_bit_identical():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, want, rinfo = _ref("ragged")
    info = {}
    got = meshrender.rasterize(_dev(v), _dev(f), mats, H, W, view_chunk=2, _info=info)       # two chunks: 2 views + 1
    _same(_np(got), want)
    npix = rinfo["npix"]
    thr = meshrender.LARGE_THRESHOLD
    assert info["skipped"] == rinfo["skipped"] == 5
    assert info["large"] == int((npix > thr).sum()) > 0 and info["small"] == int(((npix > 0) & (npix <= thr)).sum()) > 0


def test_draw_paths_agree_and_runs_repeat():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, want, rinfo = _ref("ragged")
    n = int((rinfo["npix"] > 0).sum())
    for thr, key in ((0, "large"), (1 << 30, "small")):
        info = {}
        got = meshrender.rasterize(_dev(v), _dev(f), mats, H, W, _large_threshold=thr, _info=info)
        assert info[key] == n and info["small"] + info["large"] == n
        _same(_np(got), want)
    a = meshrender.rasterize(_dev(v), _dev(f), mats, H, W)
    b = meshrender.rasterize(_dev(v), _dev(f), mats, H, W)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["tilt45", "tilt80", "ridge"])
def test_sheets_see_all_their_vertices(name):
    from neuraludf_amd import meshrender
    v, f, mats, H, W, want, info = _ref(name)
    vis = meshrender.vertex_visibility(_dev(v), _dev(f), mats, H, W, min_gap=S.VIS_GAP)
    assert vis.dtype == torch.uint8 and vis.shape == (1, len(v))
    scr = info["scr"][0]
    px, py = np.rint(scr[:, 0]), np.rint(scr[:, 1])
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    got = vis.cpu().numpy()
    assert np.array_equal(got[0] == 1, inside)
    assert np.array_equal(got, R.visible(info["scr"], want[0], S.VIS_GAP))


def test_parallel_sheets_visibility():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, want, info = _ref("parallel")
    n_front = len(v) // 2
    vis = meshrender.vertex_visibility(_dev(v), _dev(f), mats, H, W, min_gap=0.2).cpu().numpy()
    assert vis[0, :n_front].all() and not vis[0, n_front:].any()          # the front camera sees the front sheet only
    assert vis[1, n_front:].all() and not vis[1, :n_front].any()          # the rear camera the back sheet only
    assert np.array_equal(vis, R.visible(info["scr"], want[0], 0.2))
    # the default gap, twice the mean edge length (0.2, 0.2 and the diagonal), tells the sheets apart as well
    gap = 2.0 * meshrender.mean_edge_length(_dev(v), _dev(f))
    assert abs(gap - 2.0 * 0.2 * (2.0 + np.sqrt(2.0)) / 3.0) < 1e-12
    auto = meshrender.vertex_visibility(_dev(v), _dev(f), mats, H, W).cpu().numpy()
    assert np.array_equal(auto, R.visible(info["scr"], want[0], gap))
    assert np.array_equal(auto, vis)


def _ramps(n, H, W):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    coef = [((0.01, 0.005, 0.1), (-0.001, 0.01, 0.2), (0.0, 0.0, 0.5)), ((0.002, 0.003, 0.3), (0.004, -0.002, 0.4),
                                                                          (0.006, 0.001, 0.05))]
    imgs = np.stack([np.stack([a * xs + b * ys + c for a, b, c in coef[i % 2]], -1) for i in range(n)])
    return imgs.astype(np.float32), coef


def test_colours_reproduce_affine_ramps():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, want, info = _ref("tilt45")
    mats2 = np.concatenate([mats, S.pinhole(55.0, 30.0, 25.0, C=(0.2, -0.1, 0.0))[None]])
    imgs, coef = _ramps(2, H, W)
    colors, n_seen = meshrender.color_vertices(_dev(v), _dev(f), mats2, _dev(imgs), min_gap=S.VIS_GAP)
    assert colors.dtype == torch.float32 and colors.shape == (len(v), 3) and n_seen.dtype == torch.int32
    colors, n_seen = colors.cpu().numpy(), n_seen.cpu().numpy()
    vis = meshrender.vertex_visibility(_dev(v), _dev(f), mats2, H, W, min_gap=S.VIS_GAP).cpu().numpy()
    scr = R.project(v, mats2)
    assert np.array_equal(n_seen, vis.sum(0).astype(np.int32))
    u, w = scr[..., 0], scr[..., 1]
    interior = ((vis == 0) | ((u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1))).all(0) & (n_seen > 0)      # no clamped tap
    assert interior.sum() > 300 and (n_seen == 2).sum() > 100
    ramp = np.stack([np.stack([a * u[i] + b * w[i] + c for a, b, c in coef[i]], -1) for i in range(2)])       # [2, V, 3]
    mean = (ramp * vis[..., None]).sum(0) / np.maximum(n_seen, 1)[:, None]
    assert np.abs(colors[interior] - mean[interior]).max() <= 1e-6
    ref_c, ref_n = R.colour(v, mats2, vis, imgs)
    assert np.array_equal(ref_n, n_seen) and np.abs(colors - ref_c).max() <= ULP32
    # with normals and a power: |n . d|^2 weights, against the restatement
    nrm = np.stack([np.sin(v[:, 0] * 3.0), np.cos(v[:, 1] * 2.0), -1.0 + 0 * v[:, 0]], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    colors, n_seen = meshrender.color_vertices(_dev(v), _dev(f), mats2, _dev(imgs), normals=_dev(nrm), power=2.0,
                                               min_gap=S.VIS_GAP)
    ref_c, ref_n = R.colour(v, mats2, vis, imgs, nrm, R.camera_positions(mats2), 2.0)
    assert np.array_equal(ref_n, n_seen.cpu().numpy()) and np.abs(colors.cpu().numpy() - ref_c).max() <= ULP32
    assert np.abs(ref_c - R.colour(v, mats2, vis, imgs)[0]).max() > 1e-4                    # the weights matter here


def test_colours_respect_occlusion():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, _, _ = _ref("parallel")
    n_front = len(v) // 2
    v = np.concatenate([v, [[50.0, 0.0, 2.5]]])                            # a vertex of no face, outside both images
    imgs = np.empty((2, H, W, 3), dtype=np.float32)
    imgs[0], imgs[1] = 0.25, 0.75
    fill = (0.1, 0.2, 0.3)
    colors, n_seen = meshrender.color_vertices(_dev(v), _dev(f), mats, _dev(imgs), min_gap=0.2, fill=fill)
    colors, n_seen = colors.cpu().numpy(), n_seen.cpu().numpy()
    assert np.all(colors[n_front:-1] == np.float32(0.75)) and np.all(colors[:n_front] == np.float32(0.25))
    assert np.all(n_seen[:-1] == 1) and n_seen[-1] == 0 and np.array_equal(colors[-1], np.asarray(fill, dtype=np.float32))
    # uint8 images are the float32 ones scaled by 255
    rng = np.random.default_rng(3)
    img8 = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    c8, n8 = meshrender.color_vertices(_dev(v), _dev(f), mats, _dev(img8), min_gap=0.2)
    cf, nf = meshrender.color_vertices(_dev(v), _dev(f), mats, _dev((img8 / 255.0).astype(np.float32)), min_gap=0.2)
    assert torch.equal(n8, nf) and float((c8 - cf).abs().max()) <= 1.0 / 255.0
    vis = meshrender.vertex_visibility(_dev(v), _dev(f), mats, H, W, min_gap=0.2).cpu().numpy()
    assert np.abs(c8.cpu().numpy() - R.colour(v, mats, vis, img8)[0]).max() <= ULP32


def test_normal_map_of_the_square():
    from neuraludf_amd import meshrender
    v, f = S.square(1.0, 2.0)
    r = meshrender.rasterize(_dev(v), _dev(f), S.SQ_P, S.SQ_H, S.SQ_W)
    nrm = np.tile([[0.0, 0.0, -1.0]], (4, 1))
    nm = meshrender.normal_map(r, _dev(f), _dev(nrm))
    assert nm.shape == (1, S.SQ_H, S.SQ_W, 3) and nm.dtype == torch.float32
    hit = (r.face >= 0).cpu().numpy()
    nm = nm.cpu().numpy()
    assert hit.sum() == 17 * 17 and np.all(nm[hit] == np.float32([0.0, 0.0, -1.0])) and np.all(nm[~hit] == 0)
    # varying vertex normals are mixed by the barycentrics and normalised
    vary = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, -1.0], [1.0, 1.0, -1.0], [0.0, 1.0, -1.0]])
    nm = meshrender.normal_map(r, _dev(f), _dev(vary)).cpu().numpy()
    bary, face = r.bary.cpu().numpy(), r.face.cpu().numpy()
    mix = (bary[hit][:, :, None] * vary[f[face[hit]]]).sum(1)
    assert np.abs(nm[hit] - mix / np.linalg.norm(mix, axis=1, keepdims=True)).max() < 1e-6


def test_empty_and_refused_inputs():
    from neuraludf_amd import meshrender
    v, f = S.square(1.0, 2.0)
    r = meshrender.rasterize(_dev(v), _dev(f[:0]), S.SQ_P, 4, 5)
    assert torch.isinf(r.depth).all() and (r.face == -1).all() and (r.bary == 0).all() and r.depth.shape == (1, 4, 5)
    r = meshrender.rasterize(_dev(v), _dev(f), S.SQ_P[:0], 4, 5)
    assert r.depth.shape == (0, 4, 5)
    assert meshrender.vertex_visibility(_dev(v[:0]), _dev(f[:0]), S.SQ_P, 4, 5).shape == (1, 0)
    for bad in (lambda: meshrender.rasterize(_dev(v), _dev(f), S.SQ_P, 0, 5),
                lambda: meshrender.rasterize(_dev(v), _dev(f), S.SQ_P[0], 4, 5),
                lambda: meshrender.rasterize(_dev(v), _dev(f), S.SQ_P, 4, 5, view_chunk=0),
                lambda: meshrender.rasterize(_dev(v), _dev(f.astype(np.int32)), S.SQ_P, 4, 5),
                lambda: meshrender.rasterize(_dev(v), _dev(f + 2), S.SQ_P, 4, 5),
                lambda: meshrender.rasterize(torch.from_numpy(v), torch.from_numpy(f), S.SQ_P, 4, 5),
                lambda: meshrender.vertex_visibility(_dev(v), _dev(f), S.SQ_P, 4, 5, min_gap=-1.0),
                lambda: meshrender.color_vertices(_dev(v), _dev(f), S.SQ_P, _dev(np.zeros((2, 4, 5, 3), np.float32))),
                lambda: meshrender.color_vertices(_dev(v), _dev(f), S.SQ_P, _dev(np.zeros((1, 4, 5, 3), np.float64))),
                lambda: meshrender.color_vertices(_dev(v), _dev(f), S.SQ_P, _dev(np.zeros((1, 4, 5, 3), np.float32)),
                                                  power=-1.0)):
        with pytest.raises(ValueError):
            bad()


def test_cli_colours_and_renders(tmp_path, capsys):
    from PIL import Image
    from neuraludf_amd import meshing, meshrender
    v, f = S.tilted_sheet(45.0)
    H, W = S.VIS_H, S.VIS_W
    mats = np.stack([S.pinhole(20.0, 32.0, 24.0), S.pinhole(20.0, 32.0, 24.0, C=(0.3, 0.0, 0.0)),
                     S.pinhole(20.0, 32.0, 24.0, C=(-0.3, 0.1, 0.0))])
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    scan = tmp_path / "dtu" / "scan1"
    os.makedirs(scan / "mask")
    os.makedirs(scan / "image")
    np.savez(scan / "cameras.npz", **{f"world_mat_{i}": P for i, P in enumerate(mats)})
    for i in range(3):
        Image.fromarray(np.full((H, W, 3), 255, dtype=np.uint8)).save(scan / "mask" / f"{i:03d}.png")
        Image.fromarray(imgs[i]).save(scan / "image" / f"{i:03d}.png")
    np.testing.assert_array_equal(meshing.load_dtu_images(tmp_path / "dtu", 1), imgs)
    meshing.write_ply(tmp_path / "in.ply", v, f)
    rv, rf = meshing.read_ply(tmp_path / "in.ply")
    out = tmp_path / "renders"
    rc = meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--dtu-dir", str(tmp_path / "dtu"), "--scan", "1",
                       "--minimal-vis", "0", "--normals", "--colour", "--render", str(out)])
    assert rc == 0
    ov, of, on, oc = meshing.read_ply(tmp_path / "out.ply", with_normals=True, with_colors=True)
    np.testing.assert_array_equal(of, rf)                                  # every vertex is inside every mask: nothing is cut
    np.testing.assert_array_equal(ov, rv)
    assert on is not None and oc is not None and oc.dtype == np.uint8 and oc.shape == (len(rv), 3)
    dv, df = _dev(rv), _dev(rf)
    want, seen = meshrender.color_vertices(dv, df, mats, _dev(imgs), normals=meshing.vertex_normals(dv, df, torch.float64))
    assert int((seen > 0).sum()) == len(rv)
    assert np.abs(oc / 255.0 - want.cpu().numpy()).max() <= 1.0 / 255.0
    r = meshrender.rasterize(dv, df, mats, H, W)
    for i in range(3):
        depth = np.load(out / f"depth_{i}.npy")
        assert depth.dtype == np.float32 and depth.shape == (H, W)
        np.testing.assert_array_equal(depth, r.depth[i].cpu().numpy())
        img = np.asarray(Image.open(out / f"normal_{i}.png"))
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        assert np.array_equal(img.any(-1), np.isfinite(depth))
    # without the new flags the file is what it was
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "plain.ply"), "--normals"]) == 0
    write_ply_before(tmp_path / "before.ply", rv, rf, meshing.vertex_normals(dv, df).cpu().numpy())
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
    with pytest.raises(SystemExit):
        meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "x.ply"), "--colour"])
    capsys.readouterr()


def test_extract_udf_mesh_returns_colours():
    """the mesher end to end on the initialised UDF network (a blob around the origin), seen from z = -2 and coloured from
    a constant image: the same mesh as without colours, and the colours color_vertices gives that mesh with its vertex
    normals -- the image's constant where a view sees the vertex, the fill elsewhere"""
    from common import build_modules
    from neuraludf_amd import meshing, meshrender
    from neuraludf_amd.models import fields
    H, W = 48, 64
    mats = S.pinhole(40.0, 32.0, 24.0, C=(0.0, 0.0, -2.0))[None]
    imgs = torch.full((1, H, W, 3), 0.625, dtype=torch.float32, device=DEV)
    udf = build_modules(fields, seed=0)["udf"].to(DEV)
    plain = meshing.extract_udf_mesh(udf, 48)
    v, f, c = meshing.extract_udf_mesh(udf, 48, color_from=(mats, imgs))
    assert len(plain) == 2 and np.array_equal(plain[0], v) and np.array_equal(plain[1], f)
    assert c.shape == (len(v), 3) and c.dtype == np.float32
    seen, filled = (c == np.float32(0.625)).all(1), (c == np.float32(0.5)).all(1)
    assert np.all(seen | filled) and seen.any()
    dv, df = _dev(v), _dev(f)
    want, n_seen = meshrender.color_vertices(dv, df, mats, imgs, normals=meshing.vertex_normals(dv, df, torch.float64))
    assert np.array_equal(c, want.cpu().numpy()) and np.array_equal(seen, n_seen.cpu().numpy() == 1)
