"""Pin the oracle against the reference code itself: the reference side of every comparison is its own output, recorded
in tests/golden/ref_vs_reference*.npz by tests/golden/make_golden_vs_reference.py (the generator runs the reference; this
file runs anywhere).  The weights are rebuilt through the drop-in modules' seeded constructors and proven to be the
fixture's by checksum."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from common import build_modules, checksum, perturb_, state_dicts, oracle_nets
from neuraludf_amd import synth
from oracle import udf_oracle as O

import importlib.util

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_vs_reference",
                                               os.path.join(HERE, "golden", "make_golden_vs_reference.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)        # the cases (constants only: the generator's main() is not run)


def _maxrel(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "ref_vs_reference.npz"))


@pytest.fixture(scope="module")
def sds(gold):
    from neuraludf_amd.models import fields
    sds = state_dicts(perturb_(build_modules(fields, seed=0)))
    for k, sd in sds.items():        # the reference's seeded weights, rebuilt
        w = float(gold["wsum_" + k])
        assert abs(checksum(sd) - w) < 1e-6 * max(1.0, abs(w)), k
    return sds


def _rays():
    return synth.make_rays(synth.make_scene("tiny"), 0, 48, seed=5)


@pytest.mark.parametrize("case", list(G.RENDER_CASES))
def test_render_matches_reference(gold, sds, case):
    rays = _rays()
    kw = G.RENDER_CASES[case]
    cfg = O.RenderCfg(n_samples=kw["n_samples"], n_importance=kw["n_importance"], n_outside=kw["n_outside"],
                      up_sample_steps=kw["up_sample_steps"], upsampling_type=kw.get("upsampling_type", "classical"),
                      use_norm_grad_for_cosine=kw.get("use_norm_grad_for_cosine", False))
    nets = oracle_nets(sds, requires_grad=True)
    out = O.render(nets, cfg, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=0.7,
                   flip_saturation=0.9)
    for k in G.RENDER_KEYS:
        assert _maxrel(out[k].detach(), torch.from_numpy(gold[f"render_{case}_out_{k}"])) < 2e-6, k

    # parameter gradients of a runner-like loss
    G.runner_loss(out, rays["true_rgb"]).backward()
    ref = G.dequantize(np.load(os.path.join(HERE, "golden", f"ref_vs_reference_grads_{case}.npz")))
    nets_with_grads = {k.split("_", 1)[0] for k in ref}
    assert {"udf", "color", "var", "beta"} <= nets_with_grads
    assert ("nerf" in nets_with_grads) == (kw["n_outside"] > 0)
    for k, entry in ref.items():
        net, n = k.split("_", 1)
        g = getattr(nets, net)[n].grad
        assert g is not None, k
        G.assert_quantized(g, entry, G.RENDER_GRAD_TOL, k)     # max|g - ref| / max(1, max|ref|) < 5e-5


@pytest.mark.parametrize("case", G.JITTER_CASES)
def test_jittered_sampling_matches_reference(gold, sds, case):
    """perturb = 1 (what every training step -- and bench.py's timed step -- runs): the reference draws `t_rand - 0.5`
    for the coarse z and a stratified `lower + (upper - lower) * rand` for the outside samples from the default generator
    (udf_renderer_blending.py:617-627), after torch.manual_seed(77).  Replaying the same draws into the oracle's `t_rand` /
    `t_rand_out` inputs must give the reference's samples and colours."""
    rays = _rays()
    kw = G.RENDER_CASES[case]
    torch.manual_seed(77)                      # the same draws, in the reference's order and shapes
    t_rand = torch.rand([48, 1]) - 0.5
    t_out = torch.rand([kw["n_outside"]]) if kw["n_outside"] > 0 else None
    cfg = O.RenderCfg(n_samples=kw["n_samples"], n_importance=kw["n_importance"], n_outside=kw["n_outside"],
                      up_sample_steps=kw["up_sample_steps"])
    nets = oracle_nets(sds)
    with torch.no_grad():
        out = O.render(nets, cfg, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=0.7,
                       flip_saturation=0.9, t_rand=t_rand, t_rand_out=t_out)
        # and it is a different render from the unperturbed one (the test would otherwise pass vacuously)
        plain = O.render(nets, cfg, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=0.7,
                         flip_saturation=0.9)
    assert float((plain["z_vals"] - out["z_vals"]).abs().max()) > 1e-3
    for k in G.JITTER_KEYS:
        assert _maxrel(out[k].detach(), torch.from_numpy(gold[f"jitter_{case}_out_{k}"])) < 2e-6, k


def test_analytic_gradient(gold, sds):
    x = torch.from_numpy(gold["agrad_x"])
    g_ref = torch.from_numpy(gold["agrad_g"])
    nets = oracle_nets(sds)
    g1 = O.udf_gradient(nets.udf, x, create_graph=False)
    g2 = O.udf_gradient_analytic(nets.udf, x)
    assert _maxrel(g1, g_ref) < 1e-6
    assert _maxrel(g2, g_ref) < 2e-5


def test_blending_and_loss_match_reference(gold, sds):
    rays, src = G.blend_inputs()
    cfg = O.RenderCfg(n_samples=24, n_importance=12, n_outside=0, up_sample_steps=3, upsampling_type="mix",
                      use_norm_grad_for_cosine=True, h_patch_size=3)
    nets = oracle_nets(sds)
    blend = dict(color_maps=src["color_maps"], w2cs=src["w2cs"], intrinsics=src["intrinsics"],
                 query_c2w=src["query_c2w"], rays_uv=rays["rays_uv"].clone())
    out = O.render(nets, cfg, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=1.0,
                   flip_saturation=1.0, blend=blend)
    ref = {k: torch.from_numpy(gold["blend_out_" + k]) for k in G.BLEND_KEYS}
    for k in ["color", "color_pixel", "patch_colors", "patch_mask", "weights"]:
        assert _maxrel(out[k].detach(), ref[k]) < 5e-6, k

    gt_patch = torch.rand(24, 49, 3, generator=torch.Generator().manual_seed(3))
    pmask = (ref["patch_mask"] > 0.3).reshape(-1, 1)
    l = O.color_loss(1.0, 1.0, 0.5, 0.2, 3, out["color_base"], out["color"], rays["true_rgb"], out["color_pixel"],
                     rays["mask"], out["patch_colors"], gt_patch, pmask.clone())
    keys = [k[len("blend_closs_"):] for k in gold.files if k.startswith("blend_closs_")]
    assert "loss" in keys
    for k in keys:
        l_ref = float(gold["blend_closs_" + k])
        assert abs(float(l[k]) - l_ref) < 1e-5 * max(1.0, abs(l_ref)), k


@pytest.mark.parametrize("kind", G.PATCH_KINDS)
def test_patch_loss_types_match_reference(gold, kind):
    """the oracle's restatement of every ColorPatchLoss error type (loss/loss.py:56-84, loss/patch_metric.py:44-67)
    against the reference class, values and gradients w.r.t. the predicted patches."""
    ref = G.dequantize(gold, "patch_grad_")
    g = torch.Generator().manual_seed(17)
    for hps in (3, 5):
        npx = (2 * hps + 1) ** 2
        N = 41
        pred = torch.rand(N, npx, 3, generator=g)
        gt = (pred + 0.1 * torch.randn(N, npx, 3, generator=g)).clamp(0, 1)
        mask = torch.rand(N, 1, generator=g) > 0.2
        l_ref = float(gold[f"patch_{kind}_{hps}_loss"])
        p2 = pred.clone().requires_grad_(True)
        l = O.patch_loss(p2, gt, mask.clone(), hps, kind=kind)
        l.backward()
        assert abs(float(l) - l_ref) < 1e-5 * max(1.0, abs(l_ref)), (kind, hps)
        G.assert_quantized(p2.grad, ref[f"{kind}_{hps}"], G.PATCH_GRAD_TOL, (kind, hps))     # max rel. 1e-4


def _assert_reference_state_dict(gold, prefix, sd):
    """the same keys, in the same order, and bit for bit the same tensors (sha-256 of dtype, shape and bytes) as the
    reference class's seeded state_dict"""
    assert list(sd) == [str(k) for k in gold[f"{prefix}_keys"]]
    for (k, v), d in zip(sd.items(), gold[f"{prefix}_digests"]):
        assert G.digest(v) == str(d), k


@pytest.mark.parametrize("case", G.RN_CASES, ids=[c["mode"] for c in G.RN_CASES])
def test_plain_rendering_network_matches_reference(gold, case):
    """oracle restatement of RenderingNetwork (fields.py:325-397; unused by the runner, kept for the call surface)
    against the reference class's outputs, and the drop-in class's seeded state_dict against the reference's."""
    from neuraludf_amd.models import fields as nf
    kw = dict(d_feature=64, d_out=3, d_hidden=48, n_layers=3, weight_norm=True, **case)
    torch.manual_seed(3)
    sd = nf.RenderingNetwork(**kw).state_dict()
    _assert_reference_state_dict(gold, "rn_" + case["mode"], sd)        # so `sd` IS the reference's seeded weights
    g = torch.Generator().manual_seed(1)
    P = 50
    pts, nrm, dirs = (torch.randn(P, 3, generator=g) for _ in range(3))
    feat = torch.randn(P, 64, generator=g)
    color, extra = O.rendering_forward(sd, pts, nrm, dirs, feat, mode=case["mode"], multires_view=case["multires_view"],
                                       squeeze_out=case["squeeze_out"])
    out0 = torch.from_numpy(gold[f"rn_{case['mode']}_out0"])
    assert _maxrel(color, out0) < 1e-6
    if case["blending_cand_views"] > 0:
        assert _maxrel(extra, torch.from_numpy(gold[f"rn_{case['mode']}_out1"])) < 1e-6
    else:
        assert extra.shape[1] == 0 and f"rn_{case['mode']}_out1" not in gold.files


@pytest.mark.parametrize("inside_outside", [False, True])
def test_sdf_network_initialises_like_the_reference(gold, inside_outside):
    """SDFNetwork (fields.py:10-112, dead code in the runner but part of the module's surface): same parameter names, order and
    seeded values as the reference class, both camera conventions of the geometric initialisation."""
    from neuraludf_amd.models import fields
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        b = fields.SDFNetwork(**G.SDF_KW, inside_outside=inside_outside)
    sb = b.state_dict()
    _assert_reference_state_dict(gold, f"sdf_{int(inside_outside)}", sb)
    b.load_state_dict({k: v.clone() for k, v in sb.items()})
