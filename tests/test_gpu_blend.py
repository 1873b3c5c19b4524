"""Blending branch (pixel / patch warp, view softmax, composites, SSIM patch loss) against the oracle
and against the committed reference fixture."""
import os

import numpy as np
import pytest
import torch

import blend_ref
from common import build_modules, perturb_, state_dicts, oracle_nets, grel
from neuraludf_amd import synth
from oracle import udf_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def rel(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


from common import smooth_images as _smooth_images  # noqa: E402


@pytest.mark.parametrize("with_bg", [False, True])
def test_blend_stagewise(dev, with_bg):
    """values and gradients of blend_and_composite at N=21, S=37, hps=3, V=8, nl=10 against the float64 reference of
    tests/blend_ref.py, with its bound (min(max(4 e_ref, floor), 1e-3), over the rays none of whose decisions is a tie).
    The samples lie on both sides of the unit sphere, so with a background the inside / background mix and d bg_in are
    held where they are not multiplied by zero.  The other shapes: tests/test_gpu_blend_matrix.py."""
    idx = blend_ref.STAGEWISE[with_bg]
    c, r = blend_ref.CASES[idx], blend_ref.reference(idx)
    assert (c["N"], c["S"], c["hps"], c["V"], c["nl"]) == (21, 37, 3, 8, 10) and (c["bg"] == "both") == with_bg
    assert float((~r["keep"]).float().mean()) <= blend_ref.RAY_TIE_CAP
    if with_bg:
        ins = r["m64"]["inside"].float().mean()
        assert 0.2 <= float(ins) <= 0.8
    vals, grads = blend_ref.launch(dev, blend_ref.make_case(idx))
    fails = []
    blend_ref.hold(blend_ref.case_id(c), r, vals, grads, [], fails)
    assert not fails, "\n".join(fails)


def test_blend_image_layouts_agree(dev):
    """channel-interleaved source images behind an NCHW view (what the reference's dataset hands over,
    dataset.py:147-149) are read in place and give bit-identical pixel / patch colours and gradients as the planar
    NCHW copy; ray counts on both sides of the 4- / 8-waves-per-ray switch."""
    from neuraludf_amd.models import blend
    g = torch.Generator().manual_seed(11)
    scene = synth.make_scene("tiny")
    S, hps = 19, 2
    src = synth.make_source_views(scene, 0, 8)
    planar = _smooth_images(8, scene.H, scene.W).to(dev)
    inter = planar.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not inter.is_contiguous() and torch.equal(inter, planar)
    for N in (9, 1030):
        r = synth.make_rays(scene, 0, N, seed=8, margin=6)
        z = torch.sort(r["near"] + (r["far"] - r["near"]) * torch.rand(N, S, generator=g), -1)[0]
        pts = (r["rays_o"][:, None] + r["rays_d"][:, None] * z[..., None]).to(dev)
        grad = torch.randn(N, S, 3, generator=g).to(dev)
        logits, w = torch.randn(N, S, 10, generator=g).to(dev), (torch.rand(N, S, generator=g) * 0.05).to(dev)
        k1, k2 = torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 25, 3, generator=g).to(dev)
        res = []
        for imgs in (planar, inter):
            lg, wd = logits.clone().requires_grad_(True), w.clone().requires_grad_(True)
            cp, pc, pmk = blend.blend_and_composite(hps, pts, lg, wd, grad, r["rays_d"].to(dev), imgs, src["w2cs"].to(dev),
                                                    src["intrinsics"].to(dev), src["query_c2w"].to(dev),
                                                    r["rays_uv"].clone().to(dev))
            ((cp * k1).sum() + (pc * k2).sum()).backward()
            res.append((cp.detach(), pc.detach(), pmk.detach(), lg.grad, wd.grad))
        for a, b in zip(*res):
            assert torch.equal(a, b)
        assert float(res[0][1].abs().max()) > 0


def test_ssim_patch_loss(dev):
    from neuraludf_amd.loss.loss import ColorLoss
    g = torch.Generator().manual_seed(6)
    for hps in (3, 5):
        npx = (2 * hps + 1) ** 2
        N = 77
        pred = torch.rand(N, npx, 3, generator=g)
        gt = (pred + 0.1 * torch.randn(N, npx, 3, generator=g)).clamp(0, 1)
        mask = torch.rand(N, 1, generator=g) > 0.2
        cb, col, rgb, cpix = [torch.rand(N, 3, generator=g) for _ in range(4)]
        pr = pred.clone().requires_grad_(True)
        ref = O.color_loss(1.0, 1.0, 0.5, 0.2, hps, cb, col, rgb, cpix, torch.ones(N, 1), pr, gt, mask.clone())
        ref["loss"].backward()
        crit = ColorLoss(1.0, 1.0, 0.5, 0.2, "l1", "ssim", hps)
        pd = pred.to(dev).requires_grad_(True)
        D = lambda t: t.to(dev)
        out = crit(D(cb), D(col), D(rgb), D(cpix), D(torch.ones(N, 1)), pd, D(gt), D(mask.clone()))
        for k in ref:
            assert abs(float(out[k]) - float(ref[k])) < 1e-5 * max(1.0, abs(float(ref[k]))), k
        out["loss"].backward()
        assert grel(pd.grad, pr.grad) < 1e-4


@pytest.mark.parametrize("kind", ["l1", "ssd", "ncc"])
def test_patch_loss_types_l1_ssd_ncc(dev, kind):
    """the patch-error types no shipped conf uses (loss/loss.py:66-73): nudf_patch_metric against the oracle, values
    of the trimmed loss and gradients w.r.t. the predicted patches; patch sizes below and above one wave of pixels."""
    from neuraludf_amd.loss.loss import ColorPatchLoss
    from neuraludf_amd.loss.patch_metric import patch_error
    g = torch.Generator().manual_seed(16)
    for hps in (1, 3, 5):
        npx = (2 * hps + 1) ** 2
        N = 53
        pred = torch.rand(N, npx, 3, generator=g)
        gt = (pred + 0.1 * torch.randn(N, npx, 3, generator=g)).clamp(0, 1)
        mask = torch.rand(N, 1, generator=g) > 0.2
        e_ref = O.patch_error(pred, gt, hps, kind)
        e = patch_error(pred.to(dev), gt.to(dev), hps, kind)
        assert rel(e, e_ref) < 1e-5, (kind, hps)
        pr = pred.clone().requires_grad_(True)
        O.patch_loss(pr, gt, mask.clone(), hps, kind=kind).backward()
        pd = pred.to(dev).requires_grad_(True)
        out = ColorPatchLoss(kind, hps)(pd, gt.to(dev), mask.clone().to(dev))
        out.backward()
        assert grel(pd.grad, pr.grad) < 1e-4, (kind, hps)
    with pytest.raises(ValueError):
        ColorPatchLoss("huber", 3)


def test_render_with_blending_matches_reference_fixture(dev):
    """full render (mix sampling + pixel + patch blending) on the committed reference fixture's inputs;
    compared on the rays whose samples did not take a different quantile bin."""
    from neuraludf_amd.models import fields
    from neuraludf_amd.models.udf_renderer_blending import UDFRendererBlending
    gold = np.load(os.path.join(HERE, "golden", "ref_mix_blend.npz"))
    mods = perturb_(build_modules(fields, seed=0))
    for m in mods.values():
        m.to(dev)
    rays = {k[4:]: torch.from_numpy(gold[k]).to(dev) for k in gold.files if k.startswith("ray_")}
    src = synth.make_source_views(synth.make_scene("tiny"), 0, 8)
    rend = UDFRendererBlending(mods["nerf"], mods["udf"], mods["var"], mods["color"], mods["beta"], n_samples=24,
                               n_importance=12, n_outside=0, up_sample_steps=3, perturb=1.0, upsampling_type="mix",
                               use_norm_grad_for_cosine=True, h_patch_size=3)
    D = lambda t: t.to(dev)
    out = rend.render(rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=0.7,
                      perturb_overwrite=0, flip_saturation=0.9, color_maps=D(src["color_maps"]), w2cs=D(src["w2cs"]),
                      intrinsics=D(src["intrinsics"]), query_c2w=D(src["query_c2w"]), rays_uv=rays["rays_uv"].clone())
    zerr = (out["z_vals"].cpu() - torch.from_numpy(gold["out_z_vals"])).abs().max(dim=1)[0]
    good = zerr < 1e-4
    assert good.float().mean() > 0.7
    for k in ["color", "color_base", "color_pixel", "patch_colors", "patch_mask", "weights", "depth"]:
        a, b = out[k].detach().cpu()[good], torch.from_numpy(gold["out_" + k])[good]
        assert rel(a, b) < 5e-4, k          # random-noise source images: 1e-4-pixel tap differences show up


def test_patch_projector_interface_per_view_warps(dev):
    """PatchProjector.pixel_warp / .patch_warp (the reference's projector API, models/patch_projector.py:21-164): shapes and
    dtypes of the per-view colours and validity masks, both image layouts, and the in-place uv rescale of patch_warp.  The
    colours and masks themselves are held against float64 in tests/test_gpu_blend_matrix.py."""
    from neuraludf_amd.models.patch_projector import PatchProjector
    g = torch.Generator().manual_seed(14)
    scene = synth.make_scene("tiny")
    N, S, hps = 19, 23, 3
    r = synth.make_rays(scene, 0, N, seed=18, margin=10)
    src = synth.make_source_views(scene, 0, 8)
    imgs = _smooth_images(8, scene.H, scene.W)
    z = torch.sort(r["near"] + (r["far"] - r["near"]) * torch.rand(N, S, generator=g), -1)[0]
    pts = r["rays_o"][:, None] + r["rays_d"][:, None] * z[..., None]
    normals = torch.nn.functional.normalize(torch.randn(N, S, 3, generator=g), dim=-1)
    D = lambda t: t.to(dev)
    proj = PatchProjector(hps)
    for hwc in (False, True):
        im = D(imgs)
        if hwc:      # the reference's dataset hands over an NCHW view of channel-interleaved memory
            im = im.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        col, msk = proj.pixel_warp(D(pts), im, D(src["intrinsics"]), D(src["w2cs"]))
        assert col.shape == (N, S, 8, 3) and msk.shape == (N, S, 8) and msk.dtype == torch.bool
        uv = D(r["rays_uv"].clone())
        pc, pm = proj.patch_warp(D(pts), uv, D(normals), im, D(src["intrinsics"][0]), D(src["intrinsics"]),
                                 D(src["query_c2w"]), D(torch.inverse(src["w2cs"])))
        assert pc.shape == (N, S, 8, 49, 3) and pm.shape == (N, S, 8, 49) and pm.dtype == torch.bool
        # uv was rescaled in place from (-1, 1) to pixels, like the reference does (patch_projector.py:75-76)
        assert rel(uv[:, 0], (r["rays_uv"][:, 0] + 1) / 2 * (scene.W - 1)) < 1e-6
        assert rel(uv[:, 1], (r["rays_uv"][:, 1] + 1) / 2 * (scene.H - 1)) < 1e-6
