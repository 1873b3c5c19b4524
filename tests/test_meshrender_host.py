"""CPU: the host side of neuraludf_amd/meshrender.py -- the cameras of a training source (dataset_views), the camera
centres, and the argument checks that need no GPU."""
import types

import numpy as np
import pytest
import torch

import meshraster_scenes as S


def test_dataset_views_are_k_times_the_inverse_pose():
    from neuraludf_amd import meshrender
    rng = np.random.default_rng(2)
    n, H, W = 3, 6, 8
    K = np.tile(np.eye(4), (n, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 50.0, 52.0, 4.0, 3.0
    pose = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        pose[i, :3, :3], pose[i, :3, 3] = q * np.sign(np.linalg.det(q)), rng.standard_normal(3)
    src = types.SimpleNamespace(intrinsics_all=torch.from_numpy(K).float(), pose_all=torch.from_numpy(pose).float(),
                                images=torch.zeros(n, H, W, 3))
    mats, images = meshrender.dataset_views(src)
    assert mats.shape == (n, 4, 4) and mats.dtype == np.float64 and images is src.images
    # a point at camera coordinates (x, y, z) lands on the pixel the intrinsics give it, at depth z
    cam = np.array([0.1, -0.2, 2.0, 1.0])
    for i in range(n):
        Kf, pf = K[i].astype(np.float32).astype(np.float64), pose[i].astype(np.float32).astype(np.float64)
        q = mats[i] @ (pf @ cam)
        np.testing.assert_allclose(q[:3], Kf[:3, :3] @ cam[:3], atol=1e-5)
        # the camera centre is the pose's translation
        np.testing.assert_allclose(meshrender.camera_positions(mats)[i], pf[:3, 3], atol=1e-5)


def test_camera_positions():
    from neuraludf_amd import meshrender
    C = (0.1, 0.0, 6.0)
    mats = np.stack([S.pinhole(35.0, 33.0, 15.5, S.REAR, C), S.pinhole(40.0, 32.0, 16.0)])
    got = meshrender.camera_positions(mats)
    np.testing.assert_allclose(got, [C, (0.0, 0.0, 0.0)], atol=1e-12)
    np.testing.assert_array_equal(got, meshrender.camera_positions(mats[:, :3, :]))       # [n, 3, 4] is accepted
    assert meshrender.camera_positions(mats[:0]).shape == (0, 3)


def test_host_tensors_and_bad_shapes_are_refused():
    from neuraludf_amd import meshrender
    v, f = S.square(1.0, 2.0)
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(ValueError, match="GPU"):
        meshrender.rasterize(v, f, S.SQ_P, 4, 5)
    with pytest.raises(ValueError, match="GPU"):
        meshrender.vertex_visibility(v, f, S.SQ_P, 4, 5)
    with pytest.raises(ValueError, match="GPU"):
        meshrender.color_vertices(v, f, S.SQ_P, torch.zeros(1, 4, 5, 3))
    with pytest.raises(ValueError):
        meshrender.camera_positions(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError):
        meshrender.normal_map((1, 2, 3), f, v)
