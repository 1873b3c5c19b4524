"""tests/composite_ref.py on the CPU: the generator's conditions over the whole composite matrix, the helper against the
oracle's own render_core, and its float64 autograd against finite differences."""
import pytest
import torch

import composite_ref as R
from common import build_modules, perturb_, state_dicts, oracle_nets
from oracle import udf_oracle as O


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_generator_conditions(idx):
    c = R.CASES[idx]
    inp, cfg, o64, g64, o32, g32 = R.reference(idx)
    nc = R.n_chunks(c["S"], c["n_out"])
    assert inp["N"] == 2 * (nc + 1) + 1 and inp["N"] % 4 != 0
    assert inp["seed_used"] - c["seed"] < 20
    m = R.margins(inp)
    assert min(m.values()) >= R.MARGIN, ("degenerate inputs", m)
    # the recipe: spacing, levels, dips
    ST = c["S"] + c["n_out"]
    span = 2.0 * min(1.0, 48.0 / ST)
    assert float(inp["z"].min()) >= 1.0 and float(inp["z"].max()) <= 1.0 + span + 1e-6
    assert bool((inp["z"][:, 1:] > inp["z"][:, :-1]).all())
    for r in range(inp["N"]):
        k = r % (nc + 1)
        dips = (inp["udf"][r] < 0.0239).nonzero().flatten().tolist()          # levels are >= 0.04 * 0.6
        if k < nc and 64 * k < c["S"]:
            assert len(dips) == 1 and dips[0] // 64 == k, (r, dips)
            assert abs(float(inp["udf"][r, dips[0]]) - 1e-4 * (1 + r)) < 1e-9
        else:
            assert dips == [], (r, dips)
    if c["n_out"]:
        assert float((inp["bg_z"][:, 0] - inp["z"][:, -1]).min()) >= 0.2
    bad = R.degenerate(inp, cfg, o64, g64)
    assert not bad, ("degenerate inputs", bad)
    # the bound the GPU matrix will use is finite and derived here, without a kernel
    for nm in R.PER_SAMPLE_VALUES + R.PER_RAY_VALUES:
        assert R.error(nm, o32[nm], o64[nm], c["S"]) < R.CAP, nm
    for nm in ("inside", "flip"):
        assert torch.equal(o32[nm].double(), o64[nm]), nm


def test_every_setting_occurs_at_five_chunks_or_more():
    late = [c for c in R.CASES if R.n_chunks(c["S"], c["n_out"]) >= 5]
    assert {c["cos_anneal"] for c in late} == {None, 0.0, 0.6, 1.0}
    assert {c["use_norm_grad"] for c in late} == {False, True}
    assert {c["alpha_type"] for c in late} == {0, 1}
    assert {c["flip_saturation"] for c in late} == {0.0, 0.9, 1.0}
    assert {c["background"] for c in late} == {False, True}


def test_every_instantiation_is_reached():
    fwd, bwd = set(), set()
    for c in R.CASES:
        for diag in (True, False):
            f, b = R.instantiation(c["S"], c["n_out"], c["s_nominal"], diag)
            fwd.add(f)
            bwd.add(b)
    assert fwd == {"composite_fwd_kernel<%d, %s>" % (n, k) for n in (1, 2, 3, 4, 5, 6, 8) for k in ("DIAG", "FULL", "plain")}
    assert bwd == {"composite_bwd_kernel<%d, %s>" % (n, k) for n in (1, 2, 3, 4, 5, 6, 8) for k in ("FULL", "ragged")}


def test_helper_in_fp32_is_the_oracles_render_core():
    """same functions on the same (z, udf, gradients, colours): the helper restates render_core's composite"""
    from neuraludf_amd import synth
    from neuraludf_amd.models import fields
    sds = state_dicts(perturb_(build_modules(fields, seed=0)))
    nets = oracle_nets(sds)
    rays = synth.make_rays(synth.make_scene("tiny"), 0, 6, seed=7)
    cfg = O.RenderCfg(n_samples=16, n_importance=0, n_outside=0, up_sample_steps=1)
    bgc = torch.tensor([0.2, 0.5, 0.9])
    ret = O.render(nets, cfg, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], cos_anneal_ratio=0.6,
                   background_rgb=bgc, flip_saturation=0.9)
    geom = dict(rays_o=rays["rays_o"], rays_d=rays["rays_d"], z=ret["z_vals"], sdist=ret["_sample_dist"], bg_z=None)
    inv_s, beta, gamma = O.inv_s_of(nets.var).reshape(1), O.beta_of(nets.beta).reshape(1), O.gamma_of(nets.beta).reshape(1)
    o = R.oracle_composite(geom, ret["udf"].detach(), ret["gradients"].detach(), ret["_sampled_color"].detach(),
                           ret["_sampled_color_base"].detach(), inv_s, beta, gamma, kind="numerical", anneal=0.6, fs=0.9,
                           background_rgb=bgc)
    pairs = dict(color="color", color_base="color_base", weights="weights", depth="depth", normals="normals",
                 wsum="weight_sum", wsum_all="weight_sum_fg_bg", vis_prob="vis_prob", alpha="alpha", alpha_plus="alpha_plus",
                 alpha_minus="alpha_minus", alpha_occ="alpha_occ", raw_occ="raw_occ", true_cos="true_cos",
                 grad_mag="gradient_mag", mid_z="mid_z_vals", dists="dists", inside="inside_sphere")
    for a, b in pairs.items():
        ref = ret[b].detach()
        assert float((o[a] - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max())), a
    assert torch.equal(o["flip"][..., None] * ret["gradients"].detach(), ret["gradients_flip"].detach())
    s = o["sums"].detach()
    ge, gn, sp = (float(ret[k].detach()) for k in ("gradient_error", "gradient_error_near_surface", "sparse_error"))
    assert abs(float(s[0] / (s[1] + 1e-5)) - ge) <= 1e-6
    assert abs(float(s[2] / (s[3] + 1e-5)) - gn) <= 1e-6
    assert abs(float(s[4] / 6) - sp) <= 1e-6 * max(1.0, sp)


@pytest.mark.parametrize("kind,anneal,use_norm", [("numerical", None, False), ("theorical", 0.6, True)])
def test_float64_autograd_passes_gradcheck(kind, anneal, use_norm):
    inp = R.make_case(3, 1, 5, n_rays=2)
    D = lambda t: t.double().clone().requires_grad_(True)
    leaves = [D(inp[k]) for k in ("udf", "grad", "color", "color_base", "inv_s", "beta", "gamma", "bg_sigma", "bg_color")]
    bgc = inp["background_rgb"].double()

    def f(*lv):
        o = R.oracle_composite(inp, *lv, kind=kind, anneal=anneal, fs=0.9, use_norm=use_norm, background_rgb=bgc,
                               s_nominal=2, sparse_scale=25.0)
        return tuple(o[k] for k in ("color", "color_base", "weights", "depth", "normals", "wsum", "wsum_all", "sums"))

    assert torch.autograd.gradcheck(f, leaves, eps=1e-7, atol=1e-6, rtol=1e-4)
