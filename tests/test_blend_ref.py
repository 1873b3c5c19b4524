"""tests/blend_ref.py on the CPU: the generator's conditions and the tie caps over the whole blend matrix, "no fp32 / float64
decision differs outside the margins", the restated geometry and view softmax against the oracle's own, and the float64
autograd against finite differences."""
import pytest
import torch

import blend_ref as R
from oracle import udf_oracle as O

IDS = [R.case_id(c) for c in R.CASES]


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=IDS)
def test_generator_conditions(idx):
    c, r = R.CASES[idx], R.reference(idx)
    inp, keep = r["inp"], r["keep"]
    cond = R.conditions(idx)
    print(R.case_id(c), cond)          # (no_pixel_view: pixel-blend samples without a view in bounds -- reported only)
    assert torch.get_default_dtype() == torch.float32
    full = R.make_case(idx)
    assert full["N"] == c["N"] and (c["N"] < 1024 or (len(r["rows"]) >= 128 and r["rows"][0] == 0 and r["rows"][-1] == c["N"] - 1))
    assert 0.2 <= cond["inside_share"] <= 0.8, cond
    if c["hps"] is not None:
        assert 0.2 <= cond["usable_share"] <= 0.8, cond
        assert cond["no_patch_view"] >= 1, cond
        assert cond["pixel_tie_share"] <= R.PIXEL_TIE_CAP, cond
        if R.npx_of(c["hps"]) > 64:
            assert cond["second_chunk_decides"] >= 1, cond
        assert float(inp["k2"].abs().max()) > 0.5
    assert cond["tie_share"] <= R.RAY_TIE_CAP, cond
    assert float(inp["w"].abs().max()) > 0.01 and float(inp["logits"].abs().max()) > 0.5
    for nm, t in list(r["v64"].items()) + list(r["g64"].items()):
        if t is not None:
            assert float(t[keep].abs().max()) > 0, nm
            # the bound the GPU matrix will use is finite and derived here, without a kernel
            e_ref = R.error((r["v32"] if nm in r["v32"] else r["g32"])[nm], t, keep)
            assert e_ref < R.CAP / R.FACTOR, (nm, e_ref)
    assert torch.equal(r["g64"]["d_logits"][..., c["V"]:], torch.zeros_like(r["g64"]["d_logits"][..., c["V"]:]))


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=IDS)
def test_no_decision_differs_between_fp32_and_float64_outside_the_margins(idx):
    c, r = R.CASES[idx], R.reference(idx)
    t, m32, m64, geo, geo32 = r["ties"], r["m32"], r["m64"], r["geo"], r["geo32"]
    assert not bool(((m32["pix"] != m64["pix"]) & ~t["pix"]).any())
    assert not bool(((m32["inside"] != m64["inside"]) & ~t["inside"]).any())
    if c["hps"] is None:
        return
    assert not bool(((m32["patch"] != m64["patch"]) & ~t["patch_pixel"]).any())
    assert not bool(((m32["patch"].all(-1) != m64["patch"].all(-1)) & ~t["view"]).any())
    assert not bool(((geo32["valid_h"] != geo["valid_h"]) & ~t["homography"]).any())
    assert not bool((((geo32["cs"] > 0) != (geo["cs"] > 0)) & ~t["flip"]).any())
    # the restated geometry is the oracle's: same masks in float64, and in fp32 wherever the decision is not a tie
    assert torch.equal(geo["pix_mask"], m64["pix"]) and torch.equal(geo["patch_mask"], m64["patch"])
    assert torch.equal(geo["inside"], m64["inside"])
    assert not bool(((geo32["patch_mask"] != m32["patch"]) & ~t["patch_pixel"]).any())
    assert not bool(((geo32["pix_mask"] != m32["pix"]) & ~t["pix"]).any())


@pytest.mark.parametrize("idx", range(len(R.WARP_CASES)))
def test_warp_cases(idx):
    r = R.warp_reference(idx)
    t, geo = r["ties"], r["geo"]
    (p64, pm64, c64, cm64), (p32, pm32, c32, cm32) = r["w64"], r["w32"]
    assert (r["inp"]["N"] * r["inp"]["S"]) % 4 != 0
    assert float(t["patch_pixel"].float().mean()) <= R.PIXEL_TIE_CAP
    assert float(t["pix"].float().mean()) <= R.RAY_TIE_CAP
    assert not bool(((pm32 != pm64) & ~t["pix"]).any())
    assert not bool(((cm32 != cm64) & ~t["patch_pixel"]).any())
    assert torch.equal(geo["pix_mask"], pm64) and torch.equal(geo["patch_mask"], cm64)
    assert 0.2 <= float(cm64.float().mean()) <= 0.8 and 0.2 <= float(pm64.float().mean()) <= 0.95
    ok = cm64 & ~t["patch_pixel"]
    assert R.error(c32[ok], c64[ok]) < R.CAP / R.FACTOR and R.error(p32[pm64 & ~t["pix"]], p64[pm64 & ~t["pix"]]) < 1e-5


def test_the_matrix_reaches_every_instantiation_and_edge():
    got = set()
    for c in R.CASES:
        got |= set(R.instantiations(c))
    want = {"patch_blend_kernel<%s,%d,%d>" % (b, pc, w) for b in ("false", "true") for pc in (1, 2) for w in (4, 8)}
    want |= {"pixel_%s_kernel<%s>" % (k, b) for k in ("blend", "composite") for b in ("false", "true")}
    assert got == want
    assert {42, 64, 69, 133} <= {c["S"] + c["n_out"] for c in R.CASES}
    assert {c["N"] % 4 == 0 for c in R.CASES} == {False, True}
    assert {c["bg"] for c in R.CASES} >= {"both", "tail", None}
    assert {c["hps"] for c in R.CASES} >= {1, 2, 3, 4, 5}
    assert any(c["V"] == 10 == c["nl"] for c in R.CASES) and any(c["V"] < 8 for c in R.CASES)
    assert any(c["V"] == c["nl"] == 8 for c in R.CASES) and any(c["hps"] and c["S"] < 4 for c in R.CASES)
    assert {c["hps"] for c in R.WARP_CASES} == {3, 5}


def test_color_blend_without_the_fp32_casts_is_the_oracles_in_fp32():
    r = R.reference(2)
    inp = r["inp"]
    pcol, pmask = O.pixel_warp(inp["pts"], inp["imgs"], inp["intrinsics"], inp["w2cs"])
    tcol, tmask = O.patch_warp(inp["pts"], inp["rays_uv"], R.flipped_normals(inp, torch.float32), inp["imgs"],
                               inp["intrinsics"][0], inp["intrinsics"], inp["query_c2w"], torch.inverse(inp["w2cs"]), 3)
    pix, _, patch, pm = O.color_blend(inp["logits"], pcol, pmask, tcol, tmask)
    pix2, patch2, pm2 = R.color_blend(inp["logits"], pcol, pmask, tcol, tmask)
    assert torch.equal(pix, pix2) and torch.equal(patch, patch2) and torch.equal(pm, pm2)


def test_default_dtype_is_restored_after_an_exception():
    with pytest.raises(ZeroDivisionError):
        with R.default_dtype(torch.float64):
            assert torch.get_default_dtype() == torch.float64
            1 / 0
    assert torch.get_default_dtype() == torch.float32


@pytest.mark.parametrize("idx", [2, 3])
def test_float64_gradients_match_central_differences(idx):
    r = R.reference(idx)
    inp, g64 = r["inp"], r["g64"]
    g = torch.Generator().manual_seed(5)

    def f(over):
        v = R.evaluate({**inp, **over}, torch.float64)[0]
        out = (v["color_pixel"] * inp["k1"].double()).sum()
        return out + (v["patch_colors"] * inp["k2"].double()).sum()

    for key, gname in (("logits", "d_logits"), ("w", "d_w"), ("bg_in", "d_bg_in"), ("bg_tail", "d_bg_tail")):
        if inp[key] is None:
            continue
        d = torch.randn(inp[key].shape, generator=g, dtype=torch.float64)
        eps = 1e-6
        fd = float(f({key: inp[key].double() + eps * d}) - f({key: inp[key].double() - eps * d})) / (2 * eps)
        an = float((g64[gname] * d).sum())
        assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (key, fd, an)
