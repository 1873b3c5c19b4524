"""Golden fixture of tests/test_oracle_vs_reference.py: the REFERENCE side of every comparison there, produced by the
reference code itself (imported read-only from /root/reference, build container only):

    python tests/golden/make_golden_vs_reference.py   ->  tests/golden/ref_vs_reference.npz
                                                          tests/golden/ref_vs_reference_grads_<case>.npz

Small networks (tests/common.py CONF) and small batches: renders with their parameter gradients, the jittered renders,
the analytic UDF gradient, blending + ColorLoss, every ColorPatchLoss type, the seeded state dicts and outputs of
RenderingNetwork / SDFNetwork, and the checkpoint layout of the reference's networks (tests/test_host_formats.py).

Kept small without loosening a comparison: state dicts that the tests compare for EXACT equality are stored as sha-256
digests of each tensor (`digest`); the parameter / patch gradients, which the tests compare with an absolute bar
T = tol * max(1, max|ref|), are stored as integer multiples of a step s = 0.4 T (`quantize`, lzma-compressed), and the
tests then demand |got - stored| < T - s / 2, which implies |got - ref| < T (`assert_quantized`)."""
import contextlib
import hashlib
import io
import lzma
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from common import build_modules, checksum, perturb_, state_dicts  # noqa: E402
from refload import load_reference  # noqa: E402
from neuraludf_amd import synth  # noqa: E402

# the cases of tests/test_oracle_vs_reference.py (the test imports them from here)
RENDER_CASES = {
    "classical_bg": dict(n_samples=32, n_importance=20, n_outside=8, up_sample_steps=5, perturb=1.0),
    "mix": dict(n_samples=32, n_importance=24, n_outside=0, up_sample_steps=5, perturb=1.0, upsampling_type="mix",
                use_norm_grad_for_cosine=True),
    "flat": dict(n_samples=32, n_importance=0, n_outside=0, up_sample_steps=1, perturb=1.0),
}
RENDER_KEYS = ["z_vals", "color", "color_base", "weights", "depth", "udf", "gradients", "normals", "vis_prob", "alpha",
               "weight_sum", "weight_sum_fg_bg", "gradient_error", "gradient_error_near_surface", "sparse_error", "true_cos",
               "alpha_occ"]
JITTER_CASES = ["classical_bg", "flat"]
JITTER_KEYS = ["z_vals", "color", "color_base", "weights", "depth", "udf", "weight_sum", "weight_sum_fg_bg"]
BLEND_KEYS = ["color", "color_pixel", "patch_colors", "patch_mask", "weights", "color_base"]
PATCH_KINDS = ["l1", "ssd", "ncc", "ssim"]
RN_CASES = [dict(mode="idr", d_in=12, multires_view=4, squeeze_out=True, blending_cand_views=0),
            dict(mode="no_normal", d_in=6, multires_view=4, squeeze_out=True, blending_cand_views=10),
            dict(mode="no_view_dir", d_in=9, multires_view=0, squeeze_out=False, blending_cand_views=0)]
SDF_KW = dict(d_in=3, d_out=257, d_hidden=64, n_layers=5, skip_in=(3,), multires=4, bias=0.6, scale=1.5, geometric_init=True,
              weight_norm=True)


RENDER_GRAD_TOL = 5e-5       # the tests' bars: max|got - ref| / max(1, max|ref|)
PATCH_GRAD_TOL = 1e-4
STEP_OF_TOL = 0.4


def digest(t):
    """sha-256 of a tensor's dtype, shape and bytes"""
    t = torch.as_tensor(t).detach().contiguous().cpu()
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def quantize(arrays, tol):
    """{name: float32 array} -> npz fields: the arrays as integer multiples of their own step STEP_OF_TOL * tol * max(1,
    max|a|), concatenated and lzma-compressed, with names, shapes, max|a| and steps"""
    names = list(arrays)
    maxabs = np.array([float(np.abs(arrays[n]).max()) for n in names])
    steps = STEP_OF_TOL * tol * np.maximum(1.0, maxabs)
    q = [np.round(arrays[n].astype(np.float64) / st).astype(np.int64).ravel() for n, st in zip(names, steps)]
    flat = np.concatenate(q)
    assert np.abs(flat).max() < 2 ** 31
    return {"names": np.array(names), "sizes": np.array([a.size for a in q]), "maxabs": maxabs, "steps": steps,
            "shapes": np.array([",".join(map(str, arrays[n].shape)) for n in names]),
            "packed": np.frombuffer(lzma.compress(flat.astype("<i4").tobytes(), preset=9 | lzma.PRESET_EXTREME), np.uint8)}


def dequantize(f, prefix=""):
    """-> {name: (values as float64 tensor, step, maxabs)} from the fields `quantize` wrote (under `prefix`)"""
    flat = np.frombuffer(lzma.decompress(f[prefix + "packed"].tobytes()), "<i4").astype(np.float64)
    out, o = {}, 0
    for n, sz, shp, st, mx in zip(f[prefix + "names"], f[prefix + "sizes"], f[prefix + "shapes"], f[prefix + "steps"],
                                  f[prefix + "maxabs"]):
        shape = tuple(int(x) for x in str(shp).split(",") if x)
        out[str(n)] = (torch.from_numpy(flat[o:o + sz].reshape(shape) * st), float(st), float(mx))
        o += sz
    return out


def assert_quantized(got, entry, tol, what):
    """the tests' bar max|got - ref| < tol * max(1, max|ref|), checked against the stored multiple of the step: the
    rounding moved every value by at most step / 2, so the bar is tightened by that much"""
    ref, step, maxabs = entry
    bar = tol * max(1.0, maxabs)
    err = float((got.detach().double() - ref).abs().max())
    assert err < bar - step / 2, (what, err, bar - step / 2)


def runner_loss(o, true_rgb):
    return ((o["color"] - true_rgb).abs().mean() + 0.5 * (o["color_base"] - true_rgb).abs().mean()
            + 0.1 * o["gradient_error"] + 0.01 * o["gradient_error_near_surface"] + 0.001 * o["sparse_error"])


def blend_inputs():
    scene = synth.make_scene("tiny")
    return synth.make_rays(scene, 0, 24, seed=9, margin=6), synth.make_source_views(scene, 0, 8)


def main():
    rf, rr, rl = load_reference()
    mods = perturb_(build_modules(rf, seed=0))
    data = {"wsum_" + k: np.float64(checksum(v)) for k, v in state_dicts(mods).items()}

    def renderer(**kw):
        return rr.UDFRendererBlending(mods["nerf"], mods["udf"], mods["var"], mods["color"], mods["beta"], **kw)

    rays = synth.make_rays(synth.make_scene("tiny"), 0, 48, seed=5)
    grads = {}
    for case, kw in RENDER_CASES.items():
        for m in mods.values():
            m.zero_grad()
        out = renderer(**kw).render(rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=0.7,
                                    perturb_overwrite=0, flip_saturation=0.9)
        for k in RENDER_KEYS:
            data[f"render_{case}_out_{k}"] = out[k].detach().numpy()
        runner_loss(out, rays["true_rgb"]).backward()
        for net in ("udf", "color", "var", "beta") + (("nerf",) if kw["n_outside"] > 0 else ()):
            for n, p in mods[net].named_parameters():
                if p.grad is not None:
                    grads.setdefault(case, {})[f"{net}_{n}"] = p.grad.numpy().copy()
    for case in JITTER_CASES:
        torch.manual_seed(77)
        out = renderer(**RENDER_CASES[case]).render(rays["rays_o"], rays["rays_d"], rays["near"], rays["far"],
                                                    cos_anneal_ratio=0.7, perturb_overwrite=-1, flip_saturation=0.9)
        for k in JITTER_KEYS:
            data[f"jitter_{case}_out_{k}"] = out[k].detach().numpy()

    x = torch.randn(257, 3, generator=torch.Generator().manual_seed(11)) * 0.6
    data["agrad_x"] = x.numpy()
    data["agrad_g"] = mods["udf"].gradient(x.clone()).squeeze(1).detach().numpy()

    brays, src = blend_inputs()
    out = renderer(n_samples=24, n_importance=12, n_outside=0, up_sample_steps=3, perturb=1.0, upsampling_type="mix",
                   use_norm_grad_for_cosine=True, h_patch_size=3).render(
        brays["rays_o"], brays["rays_d"], brays["near"], brays["far"], cos_anneal_ratio=1.0, perturb_overwrite=0,
        flip_saturation=1.0, color_maps=src["color_maps"], w2cs=src["w2cs"], intrinsics=src["intrinsics"],
        query_c2w=src["query_c2w"], rays_uv=brays["rays_uv"].clone())
    for k in BLEND_KEYS:
        data["blend_out_" + k] = out[k].detach().numpy()
    gt_patch = torch.rand(24, 49, 3, generator=torch.Generator().manual_seed(3))
    pmask = (out["patch_mask"].detach() > 0.3).reshape(-1, 1)
    crit = rl.ColorLoss(color_base_weight=1.0, color_weight=1.0, color_pixel_weight=0.5, color_patch_weight=0.2,
                        pixel_loss_type="l1", patch_loss_type="ssim", h_patch_size=3)
    cl = crit(out["color_base"], out["color"], brays["true_rgb"], out["color_pixel"], brays["mask"], out["patch_colors"],
              gt_patch, pmask.clone())
    for k in cl:
        data["blend_closs_" + k] = np.float64(float(cl[k]))

    patch_grads = {}
    for kind in PATCH_KINDS:
        g = torch.Generator().manual_seed(17)
        for hps in (3, 5):
            npx = (2 * hps + 1) ** 2
            pred = torch.rand(41, npx, 3, generator=g)
            gt = (pred + 0.1 * torch.randn(41, npx, 3, generator=g)).clamp(0, 1)
            mask = torch.rand(41, 1, generator=g) > 0.2
            p1 = pred.clone().requires_grad_(True)
            loss = rl.ColorPatchLoss(kind, hps)(p1, gt, mask.clone())
            loss.backward()
            data[f"patch_{kind}_{hps}_loss"] = np.float64(float(loss))
            patch_grads[f"{kind}_{hps}"] = p1.grad.numpy()

    for case in RN_CASES:
        torch.manual_seed(3)
        net = rf.RenderingNetwork(d_feature=64, d_out=3, d_hidden=48, n_layers=3, weight_norm=True, **case)
        sd = net.state_dict()
        data[f"rn_{case['mode']}_keys"] = np.array(list(sd))
        data[f"rn_{case['mode']}_digests"] = np.array([digest(v) for v in sd.values()])
        g = torch.Generator().manual_seed(1)
        pts, nrm, dirs = (torch.randn(50, 3, generator=g) for _ in range(3))
        out = net(pts, nrm, dirs, torch.randn(50, 64, generator=g))
        for i, o in enumerate(out if case["blending_cand_views"] > 0 else (out,)):
            data[f"rn_{case['mode']}_out{i}"] = o.detach().numpy()

    for io_ in (False, True):
        torch.manual_seed(3)
        with contextlib.redirect_stdout(io.StringIO()):
            sd = rf.SDFNetwork(**SDF_KW, inside_outside=io_).state_dict()
        data[f"sdf_{int(io_)}_keys"] = np.array(list(sd))
        data[f"sdf_{int(io_)}_digests"] = np.array([digest(v) for v in sd.values()])

    # the layout a checkpoint of the reference's modules has (tests/test_host_formats.py): state-dict keys, parameter order
    # (the optimizer state's indices) and the seed-0 values, by checksum
    for k, m in build_modules(rf, seed=0).items():
        data[f"layout_{k}_keys"] = np.array(list(m.state_dict()))
        data[f"layout_{k}_params"] = np.array([n for n, _ in m.named_parameters()])
        data[f"layout_{k}_wsum"] = np.float64(checksum(m.state_dict()))

    data.update({"patch_grad_" + k: v for k, v in quantize(patch_grads, PATCH_GRAD_TOL).items()})
    paths = [os.path.join(HERE, "ref_vs_reference.npz")]
    np.savez_compressed(paths[0], **data)
    for case, g in grads.items():
        paths.append(os.path.join(HERE, f"ref_vs_reference_grads_{case}.npz"))
        np.savez(paths[-1], **quantize(g, RENDER_GRAD_TOL))
    for path in paths:
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
