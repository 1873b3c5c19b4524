"""The blending kernels (csrc/blend.hip) and the ray-batch kernels (csrc/raybatch.hip) may not depend on memory nobody wrote.

All outputs of models/blend.py (pix, d_logits, out, d_w, d_pix, d_in, d_tail, pc, pm, d_ws) and the six of
dataset/ray_batch.py are torch.empty.  Each case runs the clean leg twice and one leg per poison of tests/scratch_poison.py
through test_gpu_scratch_poison._legs; every output must hold the same bits (SP.same_bits) as the leg filled with 0.0 and the
status word stays 0.  The clean leg is held to the operator's own reference at the bars its own test file uses
(blend_ref.hold: the bound of test_gpu_blend_matrix.py; test_rays_oracle / rays_oracle: the figures of test_gpu_raybatch.py).

Blend cases: N = 37 rays, S = 27 samples + 8 outside, V = 3 views of the tiny scene, hps 1 and 3, planar and interleaved
images, with and without bg_in / bg_tail.  What makes these kernels skip work is asserted ON THE FLOAT64 REFERENCE
(blend_ref.evaluate / geometry), never on the kernel's output:
  * a sample no source view sees, and one that exactly one view sees (pixel blend: the masked softmax with T = 0 / one term);
  * a ray whose patch_mask is 0 and one whose patch_mask is 1: rays 0 and 1 carry all their weight on one sample, ray 0 on a
    sample none of whose views is usable, ray 1 on a sample with a usable view, so the reference's value is exactly 0 and 1;
  * a patch tap that lies in front of a source camera but off its image, on a ray that is otherwise valid (patch_mask > 0).
The cases without backgrounds have no outside samples (n_out = 0, weights [N, S]): the composite kernel multiplies the outside
weights with bg_tail and with nothing else (blend_ref.make_case ties n_out > 0 to bg_tail in the same way), so the tail
(ray, i >= S) of pixel_composite's backward -- d_w[:, S:], d_bg_tail -- and the patch launch's ldw > S are poisoned in the
bg_in_tail cases only.
Float -> index: bilinear3 clamps every tap to the image and (int)floorf saturates; ray batching indexes with the caller's integer
pixels and bounds-tests each tap (DESIGN.md section 4.1l has the rows)."""
import functools

import numpy as np
import pytest
import torch

import blend_ref as R
import scratch_poison as SP
from test_gpu_scratch_poison import _legs

pytestmark = pytest.mark.gpu

N, S, N_OUT, V, NL = 37, 27, 8, 3, 10
SEEDS = {1: 4201, 3: 4400}            # chosen on the CPU so that the reference meets the conditions (blend_conditions)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def blend_case(hps, bg):
    """fp32 inputs in blend_ref's layout and their reference (as blend_ref.reference forms it) -> dict.  Shared: callers
    leave the tensors unchanged."""
    seed = SEEDS[hps]
    g = torch.Generator().manual_seed(seed)
    inp = R._scene_inputs(N, S, V, hps, seed, g)
    w = torch.rand(N, S + N_OUT, generator=g) * 0.05
    inp.update(nl=NL, n_out=N_OUT, grad=torch.randn(N, S, 3, generator=g), logits=torch.randn(N, S, NL, generator=g),
               bg_in=torch.rand(N, S, 3, generator=g) if bg else None,
               bg_tail=torch.rand(N, N_OUT, 3, generator=g) if bg else None,
               k1=torch.randn(N, 3, generator=g), k2=torch.randn(N, R.npx_of(hps), 3, generator=g))
    if not bg:                       # without bg_tail the outside weights have nothing to multiply (blend_ref.make_case)
        w = w[:, :S].contiguous()
        inp["n_out"] = 0
    inp["w"] = w
    geo, geo32 = R.geometry(inp), R.geometry(inp, torch.float32)
    t = R.ties(inp, geo, geo32=geo32)
    usable = geo["patch_mask"].all(-1)                                                  # [N,S,V]: every patch pixel valid
    robust = ~t["view"].any(-1) & ~t["flip"]                                            # [N,S]
    any_view = usable.any(-1)
    # ray 0: all weight on a sample with no usable view; ray 1: all weight on a sample with one
    picks = []
    for ray, want in ((0, False), (1, True)):
        s = torch.nonzero((any_view[ray] == want) & robust[ray]).reshape(-1)
        assert len(s), ("ray %d has no robust sample with any_view == %s: choose another seed" % (ray, want))
        w[ray] = 0.0
        w[ray, int(s[len(s) // 2])] = 1.0
        picks.append(int(s[len(s) // 2]))
    v64, g64, m64 = R.evaluate(inp, torch.float64)
    v32, g32, m32 = R.evaluate(inp, torch.float32)
    return dict(inp=inp, rows=torch.arange(N), geo=geo, geo32=geo32, ties=t, keep=R.kept_rays(inp, t), v64=v64, g64=g64,
                m64=m64, v32=v32, g32=g32, m32=m32, picks=picks)


def blend_conditions(r):
    """the branches that skip work, counted on the float64 reference"""
    m64, v64, keep = r["m64"], r["v64"], r["keep"]
    seen = m64["pix"].sum(-1)                                                           # [N,S] views that see the sample
    pm = v64["patch_mask"]
    geo = r["geo"]                                       # in front of the camera (t2 > 0) and outside [h, W - h) x [h, H - h)
    assert torch.equal(geo["patch_mask"], m64["patch"])
    tap_out = ((geo["t2"] > 0) & ~m64["patch"]).any(-1).any(-1).any(-1)                 # [N]
    return dict(unseen=int((seen == 0).sum()), seen_by_one=int((seen == 1).sum()), pm_zero=int((pm == 0).sum()),
                pm_one=int((pm == 1).sum()), tap_off_image_on_valid_ray=int((tap_out & (pm > 0)).sum()),
                kept=int(keep.sum()), pm_zero_kept=int(((pm == 0) & keep).sum()), pm_one_kept=int(((pm == 1) & keep).sum()))


@pytest.mark.parametrize("bg", [False, True], ids=["no_bg", "bg_in_tail"])
@pytest.mark.parametrize("hwc", [False, True], ids=["planes", "hwc"])
@pytest.mark.parametrize("hps", [1, 3])
def test_blend_and_its_backward_do_not_depend_on_unwritten_memory(dev, hps, hwc, bg):
    """color_pixel, patch_colors, patch_mask and the gradients with respect to logits, weights, bg_in, bg_tail of
    blend.blend_and_composite"""
    r = blend_case(hps, bg)
    cond = blend_conditions(r)
    tag = "blend hps=%d %s %s" % (hps, "hwc" if hwc else "planes", "bg" if bg else "no bg")
    print(tag, cond)
    assert cond["unseen"] >= 1 and cond["seen_by_one"] >= 1, cond
    assert cond["pm_zero"] >= 1 and cond["pm_one"] >= 1 and cond["pm_zero_kept"] >= 1 and cond["pm_one_kept"] >= 1, cond
    assert cond["tap_off_image_on_valid_ray"] >= 1, cond
    assert float((~r["keep"]).float().mean()) <= R.RAY_TIE_CAP, cond
    assert float(r["v64"]["patch_mask"][0]) == 0.0 and float(r["v64"]["patch_mask"][1]) == 1.0

    def run():
        vals, grads = R.launch(dev, r["inp"], hwc=hwc)
        out = {"value " + k: v for k, v in vals.items() if v is not None}
        out.update({"gradient " + k: v for k, v in grads.items() if v is not None})
        return out

    clean, bad = _legs(run, dev, (), tag, differ=SP.same_bits_names, equal=SP.same_bits)
    want = {"value color_pixel", "value patch_colors", "value patch_mask", "gradient d_logits", "gradient d_w",
            "gradient d_w_patch"} | ({"gradient d_bg_in", "gradient d_bg_tail"} if bg else set())
    assert set(clean) == want, sorted(set(clean) ^ want)
    fails, rows = [], []
    R.hold(tag, r, {k[6:]: v for k, v in clean.items() if k.startswith("value ")},
           {k[9:]: v for k, v in clean.items() if k.startswith("gradient ")}, rows, fails)
    assert len(rows) == len(want) - 1                                    # (d_w_patch is the patch launch's share of d_w)
    assert not fails, "\n".join(fails)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# ray batching
# ---------------------------------------------------------------------------------------------------------------------
RB_H, RB_W, RB_IMAGES, RB_HPS = 12, 16, 3, 3


@functools.lru_cache(maxsize=None)
def raybatch_case():
    """3 images of 16 x 12 with masks, their cameras, and 37 pixels: the four corners, one pixel on each border, the four
    pixels whose 7 x 7 patch just fits or just does not, the rest drawn"""
    rng = np.random.default_rng(1612)
    H, W = RB_H, RB_W
    images = rng.integers(0, 256, (RB_IMAGES, H, W, 3)).astype(np.float32) / np.float32(256)
    masks = np.repeat((rng.random((RB_IMAGES, H, W, 1)) > 0.4).astype(np.float32), 3, -1)
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 28.9, 28.8, 7.6, 5.7
    poses = []
    for a in (0.7, -0.4, 2.1):
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        pose[:3, 3] = [1.5 * np.cos(a), -0.4, 2.0 * np.sin(a)]
        poses.append(pose)
    fixed = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1),                   # corners
             (5, 0), (9, H - 1), (0, 4), (W - 1, 7),                           # one per border
             (RB_HPS, RB_HPS), (RB_HPS + 1, RB_HPS + 1), (W - RB_HPS - 1, H - RB_HPS - 1), (W - RB_HPS, H - RB_HPS)]
    px = np.concatenate([[p[0] for p in fixed], rng.integers(0, W, 37 - len(fixed))]).astype(np.int64)
    py = np.concatenate([[p[1] for p in fixed], rng.integers(0, H, 37 - len(fixed))]).astype(np.int64)
    return dict(images=images, masks=masks, K=np.stack([K] * RB_IMAGES), poses=np.stack(poses), px=px, py=py)


@pytest.mark.parametrize("crop_patch", [False, True], ids=["no_patch", "crop_patch"])
@pytest.mark.parametrize("with_near_far", [False, True], ids=["no_near_far", "near_far"])
def test_ray_batches_do_not_depend_on_unwritten_memory(dev, with_near_far, crop_patch):
    """every output of RayBatchSource.rays_at_pixels over the three images; the clean leg against oracle/rays_oracle.py at
    the figures of test_gpu_raybatch.test_full_size_vs_oracle"""
    from neuraludf_amd.dataset import RayBatchSource
    from oracle import rays_oracle as ro
    c = raybatch_case()
    px, py = torch.from_numpy(c["px"]), torch.from_numpy(c["py"])
    assert len(px) == 37
    made = {}

    def run():
        src = made["src"] = RayBatchSource(c["images"], c["masks"], c["K"], c["poses"], device=dev)    # built under the poison
        out = {}
        for i in range(RB_IMAGES):
            s = src.rays_at_pixels(i, px, py, RB_HPS, crop_patch, with_near_far)
            out.update({"image %d %s" % (i, k): v.detach().clone() for k, v in s.items() if v is not None})
        return out

    tag = "ray batch %s %s" % ("near/far" if with_near_far else "no near/far", "crop" if crop_patch else "no crop")
    clean, bad = _legs(run, dev, (), tag, differ=SP.same_bits_names, equal=SP.same_bits)
    names = {"rays", "rays_ndc_uv", "rays_norm_XYZ_cam"} | ({"near", "far"} if with_near_far else set()) | \
            ({"rays_patch_color", "rays_patch_mask"} if crop_patch else set())
    assert set(clean) == {"image %d %s" % (i, k) for i in range(RB_IMAGES) for k in names}
    kinv = made["src"].intrinsics_all_inv.cpu().numpy()
    for i in range(RB_IMAGES):
        s = {k: clean["image %d %s" % (i, k)].cpu().numpy() for k in names}
        o = ro.gen_rays_patches(c["images"][i], c["masks"][i], kinv[i], c["poses"][i], c["px"], c["py"], RB_HPS, crop_patch)
        np.testing.assert_array_equal(s["rays"][:, 6:], o["rays"][:, 6:])
        np.testing.assert_array_equal(s["rays"][:, :3], o["rays"][:, :3])
        np.testing.assert_array_equal(s["rays_ndc_uv"], o["rays_ndc_uv"])
        np.testing.assert_allclose(s["rays"][:, 3:6], o["rays"][:, 3:6], atol=3e-7)
        np.testing.assert_allclose(s["rays_norm_XYZ_cam"], o["rays_norm_XYZ_cam"], atol=3e-7)
        if crop_patch:
            # the branch that skips work, from the oracle: patches cropped at the border (mask False) and whole ones
            assert o["rays_patch_mask"].dtype == np.bool_
            assert 0 < int(o["rays_patch_mask"].sum()) < len(px) and not o["rays_patch_mask"][:8].any()
            np.testing.assert_array_equal(s["rays_patch_mask"], o["rays_patch_mask"])
            np.testing.assert_allclose(s["rays_patch_color"], o["rays_patch_color"], atol=3e-6)
        if with_near_far:
            on, of = ro.near_far_from_sphere(o["rays"][:, :3], o["rays"][:, 3:6])
            np.testing.assert_allclose(s["near"], on, atol=2e-6)
            np.testing.assert_allclose(s["far"], of, atol=2e-6)
    assert not bad, "\n".join(bad)
