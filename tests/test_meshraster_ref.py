"""CPU: the numpy restatement of the rasteriser (tests/meshraster_ref.py) pinned on scenes with known answers
(tests/meshraster_scenes.py), before the GPU tests compare the kernels against it."""
import numpy as np
import pytest

import meshraster_ref as R
import meshraster_scenes as S


def _inside(scr, H, W):
    px, py = np.rint(scr[:, 0]), np.rint(scr[:, 1])
    return (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)


def test_fronto_parallel_square():
    verts, faces = S.square(1.0, 2.0)
    depth, face, bary = R.rasterize(verts, faces, S.SQ_P, S.SQ_H, S.SQ_W)
    ys, xs = np.mgrid[0:S.SQ_H, 0:S.SQ_W]
    covered = (xs >= 8) & (xs <= 24) & (ys >= 4) & (ys <= 20)            # the analytic set, edges inclusive
    assert np.array_equal(face[0] >= 0, covered)
    assert np.all(depth[0][covered] == 2.0) and np.all(np.isinf(depth[0][~covered]))
    diagonal = covered & (xs - 8 == ys - 4)
    assert diagonal.sum() == 17 and np.all(face[0][diagonal] == 0)      # the shared edge: the smaller face index
    assert np.all(face[0][covered & (xs - 8 > ys - 4)] == 0) and np.all(face[0][covered & (xs - 8 < ys - 4)] == 1)
    assert np.abs(bary[0][covered].sum(-1) - 1.0).max() <= 1e-6
    assert np.all(bary[0][covered] >= 0) and np.all(bary[0][~covered] == 0)


def test_smaller_square_in_front_wins_its_own_pixels():
    verts, faces = S.two_squares()
    depth, face, _ = R.rasterize(verts, faces, S.SQ_P, S.SQ_H, S.SQ_W)
    ys, xs = np.mgrid[0:S.SQ_H, 0:S.SQ_W]
    front = (xs >= 12) & (xs <= 20) & (ys >= 8) & (ys <= 16)
    back = (xs >= 8) & (xs <= 24) & (ys >= 4) & (ys <= 20) & ~front
    assert np.array_equal(face[0] >= 2, front)
    assert np.all(depth[0][front] == 1.0) and np.all(depth[0][back] == 2.0)
    assert np.array_equal((face[0] == 0) | (face[0] == 1), back)


@pytest.mark.parametrize("name", ["tilt45", "tilt80", "ridge"])
def test_a_sheet_never_hides_its_own_vertices(name):
    verts, faces = dict(tilt45=lambda: S.tilted_sheet(45.0), tilt80=lambda: S.tilted_sheet(80.0), ridge=S.ridge_sheet)[name]()
    assert len(faces) == 800 and verts[:, 2].min() >= 2.0 and verts[:, 2].max() <= 4.0
    info = {}
    depth, _, _ = R.rasterize(verts, faces, S.VIS_P, S.VIS_H, S.VIS_W, info)
    vis = R.visible(info["scr"], depth, S.VIS_GAP)
    inside = _inside(info["scr"][0], S.VIS_H, S.VIS_W)
    assert 300 < inside.sum() < len(verts)                                # some vertices project outside the image
    assert np.all(vis[0][inside] == 1) and not vis[0][~inside].any()


def test_parallel_sheets_hide_each_other():
    verts, faces, mats, n_front = S.parallel_sheets()
    info = {}
    depth, _, _ = R.rasterize(verts, faces, mats, S.VIS_H, S.VIS_W, info)
    vis = R.visible(info["scr"], depth, 0.2)
    assert vis[0, :n_front].all() and not vis[0, n_front:].any()
    assert vis[1, n_front:].all() and not vis[1, :n_front].any()


def test_ragged_scene_has_what_the_gpu_test_needs():
    verts, faces, mats, skipped = S.ragged()
    info = {}
    _, face, _ = R.rasterize(verts, faces, mats, S.RAG_H, S.RAG_W, info)
    npix = info["npix"]
    assert info["skipped"] == skipped == 5
    assert (npix > 64).any() and ((npix > 0) & (npix <= 64)).any()       # both draw lists
    assert np.all(npix[:, -3:] == 0) and npix[0, -5] == 0 and npix[2, -5] > 0 and np.all(npix[:, -4] > 0)
    assert all((face[i] >= 0).sum() > 400 for i in range(3))


def test_colour_restatement_reproduces_a_ramp():
    verts, faces = S.tilted_sheet(45.0)
    H, W = S.VIS_H, S.VIS_W
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = np.stack([0.01 * xs + 0.005 * ys + 0.1, 0.2 - 0.001 * xs + 0.01 * ys, 0.5 + 0 * xs], -1)[None]
    info = {}
    depth, _, _ = R.rasterize(verts, faces, S.VIS_P, H, W, info)
    vis = R.visible(info["scr"], depth, S.VIS_GAP)
    colors, n_seen = R.colour(verts, S.VIS_P, vis, ramp)
    u, w = info["scr"][0, :, 0], info["scr"][0, :, 1]
    interior = (vis[0] == 1) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)     # no clamped tap
    want = np.stack([0.01 * u + 0.005 * w + 0.1, 0.2 - 0.001 * u + 0.01 * w, 0.5 + 0 * u], -1)
    assert interior.sum() > 300 and np.abs(colors[interior] - want[interior]).max() <= 1e-6
    assert np.array_equal(n_seen, vis[0].astype(np.int32))
    assert np.all(colors[vis[0] == 0] == 0.5)
