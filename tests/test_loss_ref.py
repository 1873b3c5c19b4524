"""tests/loss_ref.py on the CPU: the float64 restatements equal the oracle's functions, their VJPs equal a central finite
difference, the generators meet their stated conditions, k has no tie, the matrix reaches every branch with and without a
mask, and the fp32 restatement alone stays inside the bar the GPU is held to (so every hand-written floor is at least the
reference's own error)."""
import math

import numpy as np
import pytest
import torch

import loss_ref as R
from oracle import udf_oracle as O

F32, F64 = torch.float32, torch.float64


def _close(a, b, tol=1e-12):
    a, b = [t.double() if torch.is_tensor(t) else torch.tensor(t, dtype=F64) for t in (a, b)]
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (a, b)


@pytest.mark.parametrize("kind", list(R.KINDS))
@pytest.mark.parametrize("hps", R.HPS)
def test_patch_error_equals_the_oracle(kind, hps):
    c = R.patch_case(hps, 257)
    for dtype in (F64, F32):
        mine = R.patch_error(c["pred"], c["gt"], c["win"], kind, dtype)
        theirs = O.patch_error(c["pred"].to(dtype), c["gt"].to(dtype), hps, kind)
        _close(mine, theirs, 1e-12 if dtype == F64 else 0.0)


def test_the_window_is_the_package_s():
    from neuraludf_amd.loss.patch_metric import gaussian_window
    for hps in R.HPS:
        assert torch.equal(R.window(hps), gaussian_window(hps))
        assert R.window(hps).dtype == F32 and len(R.window(hps)) == R.npx_of(hps)


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_patch_vjp_equals_a_central_difference(kind):
    c = R.patch_case(3, 5)
    g = torch.Generator().manual_seed(1)
    err, grad = R.patch_error_vjp(c["pred"], c["gt"], c["win"], kind, c["d_out"], F64)
    v = torch.randn(c["pred"].shape, generator=g, dtype=F64)
    if kind == "l1":
        v = v * c["l1_keep"] * (c["pred"] != c["gt"])        # |x| has no derivative at 0; autograd's 0 there is checked below
    h = 1e-7
    f = lambda p: float((R.patch_error(p, c["gt"], c["win"], kind, F64) * c["d_out"].double()).sum())
    fd = (f(c["pred"].double() + h * v) - f(c["pred"].double() - h * v)) / (2 * h)
    assert abs(fd - float((grad * v).sum())) <= 1e-6 * max(1.0, float((grad * v).abs().sum()))
    assert bool((grad[c["zero"]] == 0).all())                # d_out == 0: the ray's gradient row is exactly zero
    if kind == "l1":
        assert bool((grad[c["pred"] == c["gt"]] == 0).all())
    # the pixel permutation behind e_ref_extra is undone in the gradient
    perm = torch.randperm(c["npx"], generator=g)
    _close(R.patch_error_vjp(c["pred"], c["gt"], c["win"], kind, c["d_out"], F64, perm=perm)[1], grad, 1e-9)


def test_color_and_step_loss_equal_the_oracle_and_a_central_difference():
    for N, mk, wname in ((65, "random", "shipped"), (63, "none", "uneven"), (255, "zeros", "no_pixel")):
        c, mask, w = R.color_case(N), R.mask_case(N, mk), R.WEIGHTS[wname]
        total, Lb, Lc, den = R.color_loss(c["cb"], c["c"], c["gt"], mask, w, F64)
        o = O.color_loss(w["base"], w["color"], w["pixel"], w["patch"], 3, c["cb"].double(), c["c"].double(), c["gt"].double(), None,
                         None if mask is None else mask.double(), None, None, None)
        _close(total, o["loss"])
        _close(Lb, o["color_base_loss"])
        _close(Lc, o["color_loss"])
        _close(den, 3 * N if mask is None else float(mask.sum()) + 1e-4)
        # the sharded form
        s = R.color_sums(c["cb"], c["c"], c["gt"], mask, F64)
        for a, b in zip(R.color_finish(s, mask is not None, w, F64), (total, Lb, Lc, den)):
            _close(a, b)
        # the step: the masked means and the runner's total
        sums = R.sums_case(0)
        out, _ = R.step_loss(c["cb"], c["c"], c["gt"], mask, sums, R.N_RAYS, w, F64)
        ge, gens, sp = float(sums[0]) / (float(sums[1]) + 1e-5), float(sums[2]) / (float(sums[3]) + 1e-5), float(sums[4]) / R.N_RAYS
        _close(out[0], float(total) + gens * w["igr_ns"] + sp * w["sparse"] + ge * w["igr"])
        _close(torch.stack(out[4:7]), torch.tensor([ge, gens, sp], dtype=F64))
        _close(R.step_loss(c["cb"], c["c"], c["gt"], mask, R.sums_case(0, 17), R.N_RAYS, w, F64)[0][0], out[0], 1e-6)
        # VJP against a central difference along a direction that avoids the kinks
        g = torch.Generator().manual_seed(N)
        d_cb, d_c, d_s = R.step_loss_vjp(c["cb"], c["c"], c["gt"], mask, sums, R.N_RAYS, w, R.D_TOTAL, R.D_EXTRA, F64)
        va = torch.randn(N, 3, generator=g, dtype=F64) * (c["cb"] != c["gt"])
        vb = torch.randn(N, 3, generator=g, dtype=F64) * (c["c"] != c["gt"])
        vs = torch.randn(5, generator=g, dtype=F64)

        def f(t):
            o8, _ = R.step_loss(c["cb"].double() + t * va, c["c"].double() + t * vb, c["gt"], mask, sums.double() + t * vs, R.N_RAYS, w, F64)
            return float(o8[0] * R.D_TOTAL + sum(o8[k] * R.D_EXTRA[k] for k in range(1, 8)))
        h = 1e-7
        an = float((d_cb * va).sum() + (d_c * vb).sum() + (d_s * vs).sum())
        assert abs((f(h) - f(-h)) / (2 * h) - an) <= 1e-5 * max(1.0, abs(an))
        assert bool((d_cb[c["cb"] == c["gt"]] == 0).all()) and bool((d_c[c["c"] == c["gt"]] == 0).all())
        # the colour loss's own upstream triple
        for d in R.D_COLOR:
            a, b = R.color_loss_vjp(c["cb"], c["c"], c["gt"], mask, w, d, F64)
            W = w["base"] + w["color"] + w["pixel"]
            _close(a, (d[0] * w["base"] / W + d[1]) / float(den) * torch.sign(c["cb"].double() - c["gt"].double()))
            _close(b, (d[0] * w["color"] / W + d[2]) / float(den) * torch.sign(c["c"].double() - c["gt"].double()))


def test_blend_loss_equals_the_oracle_and_a_central_difference():
    N, hps = 257, 1
    pc = R.patch_case(hps, N)
    err = R.patch_error(pc["pred"], pc["gt"], pc["win"], "ssim", F32) + 0.01
    for count, wname in (("0.6N", "shipped"), ("4", "uneven"), ("N", "no_pixel")):
        c, w = dict(R.blend_case(N, count)), R.WEIGHTS[wname]
        a = (c["cb"], c["c"], c["pix"], c["gt"], c["err"], c["patch_mask"], c["weight_sum"], R.sums_case(2), R.N_RAYS, w, R.RATIO)
        r = R.blend_loss(*a, F64)
        m = (c["patch_mask"][:, None] * (c["weight_sum"][:, None] > 0.5).float()) > 0
        assert torch.equal(r["m"], m[:, 0]) and int(m.sum()) == c["n_valid"]
        # the oracle's patch_loss on errors of its own: the trim and the mean
        D = lambda t: t.double()
        lt = O.patch_loss(D(pc["pred"]), D(pc["gt"]), m, hps, R.RATIO, "ssim")
        mine = R.blend_loss(*a[:4], R.patch_error(pc["pred"], pc["gt"], pc["win"], "ssim", F64), *a[5:], F64)
        _close(mine["out"][5], lt)
        o = O.color_loss(w["base"], w["color"], w["pixel"], w["patch"], hps, D(c["cb"]), D(c["c"]), D(c["gt"]), D(c["pix"]), None,
                         D(pc["pred"]), D(pc["gt"]), m)
        _close(mine["out"][1], o["loss"])
        _close(mine["out"][4], o["color_pixel_loss"])
        _close(mine["out"][2], o["color_base_loss"])
        assert r["k"] == int(R.RATIO * m.sum()) == c["k"] and r["kept"] == c["n_valid"] - c["k"]
        assert int(r["keep"].sum()) == r["kept"] and not bool(r["keep"][~m[:, 0]].any())
        # central difference
        g = torch.Generator().manual_seed(3)
        grads = R.blend_loss_vjp(*a, R.D_TOTAL, F64)
        vs = [torch.randn(N, 3, generator=g, dtype=F64) * (c[k] != c["gt"]) for k in ("cb", "c", "pix")]
        ve, v5 = torch.randn(N, generator=g, dtype=F64), torch.randn(5, generator=g, dtype=F64)

        def f(t):
            rr = R.blend_loss(D(c["cb"]) + t * vs[0], D(c["c"]) + t * vs[1], D(c["pix"]) + t * vs[2], c["gt"], D(c["err"]) + t * ve,
                              c["patch_mask"], c["weight_sum"], D(R.sums_case(2)) + t * v5, R.N_RAYS, w, R.RATIO, F64)
            return float(rr["out"][0]) * R.D_TOTAL
        h = 1e-8                                        # (below the gaps between the sorted errors: the kept set stays)
        an = float(sum((gr * v).sum() for gr, v in zip(grads, vs + [ve, v5])))
        assert abs((f(h) - f(-h)) / (2 * h) - an) <= 1e-4 * max(1.0, abs(an))
        assert torch.equal(grads[3] != 0, r["keep"])     # d_err is non-zero exactly on the kept rays


def test_the_empty_selection_is_nan_in_the_reference():
    r = R.blend_rows(10, "0", "shipped", 0, 0)
    assert set(r["_nan"]) == {"out0", "out1", "out5"}
    assert r["_ref"]["k"] == 0 and r["_ref"]["kept"] == 0
    assert bool((r["d_err"]["r64"] == 0).all()) and bool(torch.isfinite(r["d_cb"]["r64"]).all())
    # (a bool mask: mask.sum() + 1e-4 is an int64 tensor plus a Python float, float32 in torch -- in the reference as well)
    assert float(r["out9"]["r64"]) == float(np.float32(1e-4))


def test_k_has_no_tie():
    """int(0.3 * count) with torch's float32 product, floor(0.3f * count) in fp32 and the double product agree for every
    count below 5000"""
    counts = torch.arange(0, 5000, dtype=torch.int64)
    a = (R.RATIO * counts).to(torch.int64)                                      # a Python float times an int64 tensor: float32
    assert (R.RATIO * counts).dtype == F32
    b = torch.floor(torch.tensor(R.RATIO, dtype=F32) * counts.float()).to(torch.int64)
    d = torch.tensor([int(R.RATIO * int(n)) for n in counts])
    assert torch.equal(a, b) and torch.equal(a, d)
    for N, count, *_ in R.BLEND_CASES:
        c = R.blend_case(N, count)
        assert R.trim_count(R.RATIO, c["n_valid"]) == int(a[c["n_valid"]]) == c["k"]
    assert R.trim_count(R.RATIO, 3) == 0 and R.trim_count(R.RATIO, 4) == 1


def test_generators_meet_their_conditions():
    assert R.RAYS == [1, 63, 64, 65, 255, 257, 999, 341, 342] and 3 * 341 == 1023 and 3 * 342 == 1026
    for N in R.RAYS:
        c = R.color_case(N)
        for nm in ("cb", "c"):
            d = (c[nm].double() - c["gt"].double()).reshape(-1)
            assert float((~c["keep_" + nm]).float().mean()) <= R.TIE_CAP
            assert int((d == 0).sum()) >= (3 * N) // 7                      # every seventh element equal, kept
            assert bool(c["keep_" + nm][d == 0].all())
        assert R.mask_case(N, "none") is None
        assert R.mask_count(N, "ones") == N and R.mask_count(N, "zeros") == 0 and R.mask_count(N, "one") == 1
        assert R.mask_case(N, "random").shape == (N, 1)
        if N >= 63:
            assert 0.4 * N < R.mask_count(N, "random") < 0.8 * N
    for hps in R.HPS:
        for N in R.PATCH_RAYS:
            c = R.patch_case(hps, N)
            assert c["pred"].shape == (N, R.npx_of(hps), 3)
            assert float((~c["l1_keep"]).float().mean()) <= R.TIE_CAP
            assert bool((c["d_out"][c["zero"]] == 0).all()) and bool((c["d_out"][~c["zero"]] != 0).all())
            if N >= 255:
                assert abs(float(c["zero"].float().mean()) - 1 / 3) < 0.02
                assert bool((c["d_out"] > 0).any()) and bool((c["d_out"] < 0).any())
            eq = torch.tensor([R.CLASSES[r % 6] == "equal" for r in range(N)])
            assert bool((c["pred"][eq] == c["gt"][eq]).all())
    assert [R.npx_of(h) for h in R.HPS] == [9, 49, 81, 121] and R.CLASSES[256 % 6] == "half"
    for N, count, *_ in R.BLEND_CASES:
        c = R.blend_case(N, count)                                        # (asserts the untied trim boundary itself)
        m = (c["patch_mask"] * (c["weight_sum"] > 0.5).float()) > 0
        want = dict(zip(R.BLEND_COUNTS, (0, 1, 3, 4, 10, int(round(0.6 * N)), N)))[count]
        assert int(m.sum()) == want == c["n_valid"]
        assert set(c["patch_mask"].tolist()) <= {0.0, 1.0}
        if N - want >= 20:
            assert bool(((c["patch_mask"] > 0) & ~m).any()) and bool(((c["weight_sum"] > 0.5) & ~m).any())
            assert bool((c["weight_sum"] == 0.5).any())
        v = c["err"][m]
        assert len(torch.unique(v)) == len(v) and bool((v > 0).all())
    for si in range(3):
        for nblk in R.NBLK:
            ws = R.sums_case(si, nblk)
            assert ws.shape == (nblk, 5) and bool((ws >= 0).all())
            _close(ws.double().sum(0), torch.tensor(R.SUMS5[si]).double(), 1e-6)


def test_the_matrix_reaches_every_branch():
    assert len(R.COLOR_CASES) == len(R.STEP_CASES) == len(R.RAYS) * len(R.MASKS)
    for masked in (False, True):
        sel = lambda cases: [c for c in cases if (c[1] != "none") == masked]
        assert {c[4] for c in sel(R.COLOR_CASES)} == {"value", "dev"}
        assert {c[3] for c in sel(R.COLOR_CASES)} == {0, 1, 2}
        st = sel(R.STEP_CASES)
        assert {c[6] for c in st} == {"value", "dev"} and {c[5] for c in st} == set(R.UPSTREAMS)
        assert {c[4] for c in st} == {0, 1, 17, 1024, 1025} and {c[2] for c in st} == set(R.WNAMES)
    assert {c[1] for c in R.BLEND_CASES} == set(R.BLEND_COUNTS)
    for count in R.BLEND_COUNTS:
        b = [c for c in R.BLEND_CASES if c[1] == count]
        assert {c[5] for c in b} == {R.D_TOTAL, None} and len({c[4] for c in b}) >= 3
    assert {c[0] for c in R.BLEND_CASES} == set(R.BLEND_RAYS)
    assert all(x != 0 for x in R.D_EXTRA[1:7])


def _hold(specs, case):
    rows, fails = [], []
    R.reference_holds(case, specs, rows, fails)
    assert not fails, "\n".join(fails[:10])
    return rows


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_the_reference_stays_inside_its_bar_patch(kind):
    for hps in R.HPS:
        for N in R.PATCH_RAYS:
            _hold(R.patch_rows(kind, hps, N), "%s_hps%d_N%d" % (kind, hps, N))


def test_the_reference_stays_inside_its_bar_color_step_blend():
    for c in R.COLOR_CASES:
        _hold(R.color_rows(*c[:4]), "color_%s" % (c,))
    for c in R.SHARD_CASES:
        _hold(R.shard_rows(*c), "shard_%s" % (c,))
    for c in R.STEP_CASES:
        _hold(R.step_rows(*c[:6]), "step_%s" % (c,))
    for c in R.BLEND_CASES:
        _hold(R.blend_rows(*c), "blend_%s" % (c,))


def test_floor_counts_are_written_down():
    assert R.HALF_ULP == 2.0 ** -24 and R.SUM == 2
    assert R.rfloor("reg", 3.0) == R.quotient_floor(3.0) * 6 / 4
    assert all(isinstance(v, int) and 0 <= v <= 16 for v in R.ROUNDINGS.values())
    assert math.isclose(R.rfloor("L", 2.0), 5 * 2.0 ** -24 * 2.0)
    assert np.float32(R.f32(0.1)) == np.float32(0.1) and R.f32(0.1) != 0.1
