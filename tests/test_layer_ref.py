"""tests/layer_ref.py checked on the CPU: every restatement against the oracle / torch autograd in float64, the generators'
conditions and tie caps on the float64 reference alone, fp32 and float64 deciding alike outside the margins, and the softplus
window's fp32 figures that the GPU bar of tests/test_gpu_layer_matrix.py rests on."""
import math

import pytest
import torch

import layer_ref as R
from oracle import udf_oracle as O

F32, F64 = R.F32, R.F64


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------ #
# restatements
# ------------------------------------------------------------------------------------------------------------------ #
def test_softplus_derivatives_are_autograds():
    """(no point at a = 0.2 itself: 100 a against the threshold 20 is a tie there, 2e-7 of softplus'' apart)"""
    a = torch.cat([torch.linspace(-0.4, 0.4, 4000, dtype=F64), torch.tensor([0.2 + 1e-9, 0.2 - 1e-9], dtype=F64)])
    a.requires_grad_(True)
    h = O.softplus100(a)
    (s,) = torch.autograd.grad(h.sum(), a, create_graph=True)
    (d2,) = torch.autograd.grad(s.sum(), a)
    close(R.sp_s(a.detach()), s.detach())
    close(R.sp_d2(a.detach()), d2, 1e-10)
    close(R.sp_s(a.detach()) + R.sp_om(a.detach()), torch.ones_like(a))
    # s recovered from the stored activation (what the s-from-h epilogues are handed) is the same s
    for xs in (1.0, 1.4142135):
        x = 100.0 * xs * R.stored(a.detach().float(), xs).double()
        s_h = torch.where(x > 20, torch.ones_like(x), -torch.expm1(-x))
        assert R.relmax(s_h, R.sp_s(a.detach().float().double())) < 2e-6


def test_udf_heads_are_the_networks():
    """fields.py:184-190 through the oracle's config: udf_forward's column 0 is the head of the last layer's column 0"""
    v = torch.randn(50, dtype=F64)
    for kind in R.HEADS.values():
        vv = v.clone().requires_grad_(True)
        hv, hm = R.udf_head(vv, kind)
        (g,) = torch.autograd.grad(hv.sum(), vv)
        close(hm.detach(), g)


def test_epilogues_cover_the_thirteen_and_every_option():
    assert sorted({v["epi"] for v in R.VARIANTS}) == sorted(R.EPILOGUES) and len(R.EPILOGUES) == 13
    from neuraludf_amd._lib import EPI
    assert sorted(EPI) == sorted(R.EPILOGUES)
    for epi in R.EPILOGUES:
        shapes = [s for v in R.VARIANTS if v["epi"] == epi for s in v["shapes"]]
        Ms, Ns, Ks = {s[0] for s in shapes}, {s[1] for s in shapes}, {s[2] for s in shapes}
        assert min(Ms) < 32 < max(m for m in Ms if m <= 64) <= 64 < max(Ms) and len(Ks) >= 2, epi
        assert min(Ns) < 32 < 64 < max(Ns) and any(32 < n <= 64 for n in Ns), epi
        assert (256, 65, 32) in shapes and (512, 130, 64) in shapes
    names = {v["name"] for v in R.VARIANTS}
    assert {"SOFTPLUS", "SOFTPLUS_c2", "BWD", "BWD_x2", "RELU_DUAL", "RELU_DUAL_c2", "SIGMOID", "SIGMOID_c2", "SIGMOID_c3",
            "SIGMOID_c2_c3", "UDFHEAD_abs", "UDFHEAD_square", "UDFHEAD_sdf", "SKIPSPLIT_25", "SKIPSPLIT_64"} <= names
    for nm in ("SIGMOID", "SIGMOID_c2", "SIGMOID_c3", "SIGMOID_c2_c3"):
        assert {s[1] for s in R.VARIANT[nm]["shapes"]} >= {3, 6, 35} and R.VARIANT[nm]["o"]["iparam"] == 3
    for nm, ip in (("SKIPSPLIT_25", 25), ("SKIPSPLIT_64", 64)):
        ns = {s[1] for s in R.VARIANT[nm]["shapes"]}
        assert any(n <= ip for n in ns) and any(ip < n <= ip + 32 for n in ns) and any(n > ip + 32 for n in ns)
    assert any(s[1] == 1 for s in R.VARIANT["UDFHEAD_abs"]["shapes"])           # udf_only: C1 == NULL


@pytest.mark.parametrize("name", [v["name"] for v in R.VARIANTS])
def test_gemm_cases_conditions_and_ties(name):
    var = R.VARIANT[name]
    shares = torch.zeros(3)
    for si, (M, N, K) in enumerate(var["shapes"]):
        c = R.gemm_case(name, si)
        assert float((~c["keep"]).float().mean()) <= R.TIE_CAP, (name, si)
        for k, r in c["r64"].items():
            assert r.dtype == F64 and c["r32"][k].dtype == F32 and r.shape == c["r32"][k].shape and bool(torch.isfinite(r).all())
            assert all(e[k].shape == r.shape for e in c["r32_extra"])
        o = c["o"]
        if "apre" in o:
            shares += torch.tensor(R.branch_shares(o["apre"], o["xscale"])) * (M * N)
        if "X1" in o and M * N >= 64:
            assert bool((o["X1"] == 0).any()) and bool((o["X1"] < 0).any()) and bool((o["X1"] > 0).any())
        if c["epi"] == "UDFHEAD" and o["iparam"] == 0:
            # fp32 and float64 agree on the sign outside the margin
            k = c["keep"]
            assert torch.equal(torch.sign(c["v32"][k, 0]).double(), torch.sign(c["v64"][k, 0]))
            if M >= 64:
                assert bool((c["v64"][:, 0] > 0).any()) and bool((c["v64"][:, 0] < 0).any())
        if c["epi"] == "SOFTPLUS":
            assert float(c["v64"].min()) > -0.8            # softplus stays inside fp32's normal range
            if M * N >= 2000:
                assert bool((100 * c["v64"] > 20).any()) and bool((c["v64"] < -0.1).any())
        if c["epi"] == "RELU" and M * N >= 64:
            assert bool((c["v64"] > 0).any()) and bool((c["v64"] < 0).any())
    if var["epi"] in R.S_FROM_H:
        shares /= shares.sum()
        assert float(shares.min()) > 0.03, shares          # all three branches of the recovery


def test_softplus_window_figures():
    """the CPU facts the window bar rests on.  torch's fp32 softplus and softplus' keep ~6e-7 of the element over
    1e-4 <= z <= 1e-2; the expression the SOFTPLUS epilogue used, z < 1e-4 ? series : log(1 + z) in fp32 with exact exp / log,
    loses 5.9e-4 at z = 1e-4; log1p(z) does not."""
    f = R.window_figures()
    assert 3e-7 < f["softplus"] < 9e-7 and 3e-7 < f["s_from_pre"] < 9e-7 and 5e-8 < f["s_from_h"] < 5e-7, f
    a = R.window_points()
    z = torch.exp(100.0 * a)
    old = torch.where(z < 1e-4, (z - 0.5 * z * z) * 0.01, torch.log(1.0 + z) * 0.01)
    assert 4e-4 < R.relmax(old, R.sp(a.double())) < 8e-4
    assert R.relmax(torch.log1p(z) * 0.01, R.sp(a.double())) < 9e-7
    # s = 1 - exp(-100 h) from that h inherits the loss; from an exact h it does not
    s_old = -torch.expm1(-100.0 * old)
    assert R.relmax(s_old, R.sp_s(a.double())) > 4e-4
    for epi in ("SOFTPLUS",) + R.S_FROM_H:
        c = R.window_case(epi)
        fig = R.relmax(c["r32"]["C1"], c["r64"]["C1"])
        assert 2e-7 < fig < 9e-7, (epi, fig)               # WINDOW_FACTOR x this is the GPU's bar for the epilogue
        zz = torch.exp(100.0 * (c["A"] if epi == "SOFTPLUS" else c["o"]["apre"]).double())
        assert float(zz.min()) >= R.WINDOW[0] and float(zz.max()) <= R.WINDOW[1]
        if epi == "SOFTPLUS":
            assert torch.equal(c["v64"], c["A"].double())
    c = R.window_case("MULSP")                             # udf_grad_seed runs on its stored activations
    assert max(R.branch_shares(c["o"]["apre"], 1.4142135)[1:]) == 0.0


# ------------------------------------------------------------------------------------------------------------------ #
def test_posenc_restatements():
    g = torch.Generator().manual_seed(0)
    for D, L in ((3, 4), (4, 10), (3, 15)):
        x = torch.randn(9, D, generator=g, dtype=F64) * 0.8
        v = torch.randn(14, D, generator=g, dtype=F64)
        E = D * (2 * L + 1)
        e = R.posenc(x, L, 0.37, 2, 14, 0.5, F64)
        assert e.shape == (14, E)
        close(e[5], O.posenc(x[2] * 0.37, L) * 0.5)
        # the JVP is the directional derivative (central differences), the VJP its transpose
        j = R.posenc_jvp(x, v, L, 0.37, 2, 14, 0.5, F64)
        xr = x.repeat_interleave(2, 0)[:14]
        h = 1e-4 / 2 ** L
        fd = (O.posenc((xr + h * v) * 0.37, L) - O.posenc((xr - h * v) * 0.37, L)) / (2 * h) * 0.5
        close(j, fd, 1e-5)
        s1, s2 = torch.randn(14, E, generator=g, dtype=F64), torch.randn(14, E, generator=g, dtype=F64)
        gr = R.posenc_vjp(xr, L, 0.37, s1, 1.0, s2, 0.7, F64)
        jv = R.posenc_jvp(xr, v, L, 0.37, 1, 14, 1.0, F64)
        close((gr * v).sum(), ((s1 + 0.7 * s2) * jv).sum(), 1e-10)
        assert R.posenc_vjp(xr.float(), L, 0.37, s1.float(), 1.0, None, 0.0, F32).dtype == F32
    close(R.copy_cols(torch.arange(12.0).reshape(4, 3), 3, 2, 10, 2.0, F64)[7], torch.tensor([12.0, 14.0], dtype=F64))


def test_sampling_restatements_are_the_oracles():
    g = torch.Generator().manual_seed(1)
    N, S = 6, 16
    near, far, tr = 1.5 + torch.rand(N, 1, generator=g), 3.5 + torch.rand(N, 1, generator=g), torch.rand(N, 1, generator=g)
    cfg = O.RenderCfg(n_samples=S, n_importance=0, n_outside=5, up_sample_steps=1)
    z, z_out, sd = O.coarse_z(cfg, near, far, N, t_rand=tr - 0.5)
    z32, sd32 = R.coarse_z(near, far, S, tr, True, F32)
    assert torch.equal(z32, z) and abs(float(sd32) - sd) < 1e-7
    lin = torch.linspace(1e-3, 1.0 - 1.0 / 6.0, 5)
    assert torch.equal(R.outside_z(far, lin, S, F32), z_out)
    z64, sd64 = R.coarse_z(near, far, S, tr, True, F64)
    assert z64.dtype == F64 and float((z64 - z.double()).abs().max()) < 1e-6
    o, d = torch.randn(N, 3, generator=g), torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    p0, p1, p2 = (R.ray_points(o, d, z, sd64, m, F64) for m in (0, 1, 2))
    close(p0.reshape(N, S, 3)[2, 5], o[2].double() + d[2].double() * z64[2, 5], 1e-6)
    mid = z.double()[2, 5] + 0.5 * (z.double()[2, 6] - z.double()[2, 5])
    close(p1.reshape(N, S, 3)[2, 5], o[2].double() + d[2].double() * mid)
    close(p1.reshape(N, S, 3)[2, S - 1], o[2].double() + d[2].double() * (z.double()[2, S - 1] + 0.5 * sd64))
    r = torch.linalg.norm(p1, dim=-1).clip(1.0, 1e10)
    close(p2, torch.cat([p1 / r[:, None], 1.0 / r[:, None]], -1))


def test_head_restatements():
    c = R.seed_case(65, 33)
    sh = R.branch_shares(c["apre"], 1.4142135)
    assert min(sh) > 0.03, sh
    out = R.udf_grad_seed(c["sign"], c["wrow"], c["apre"], 0.77, F64)
    # d/da of sign * inv_scale * (softplus(a) . wrow)
    a = c["apre"].double().requires_grad_(True)
    (c["sign"].double() * 0.77 * (O.softplus100(a) @ c["wrow"].double())).sum().backward()
    close(out, a.grad)
    g = torch.Generator().manual_seed(2)
    sign, dudf, dfeat = torch.sign(torch.randn(7, generator=g)), torch.randn(7, generator=g), torch.randn(7, 4, generator=g)
    # adjoint of y = [|v0| scale, v1..]: d v = [sign scale dudf, dfeat]
    v = torch.randn(7, 5, generator=g, dtype=F64)
    v[:, 0] = v[:, 0].abs() * sign.double()
    v.requires_grad_(True)
    ((v[:, 0].abs() * 1.3 * dudf.double()).sum() + (v[:, 1:] * dfeat.double()).sum()).backward()
    close(R.udf_head_bwd(sign, dudf, dfeat, 1.3, 7, 4, F64), v.grad)
    assert float(R.udf_head_bwd(sign, None, dfeat, 1.3, 7, 4, F64)[:, 0].abs().max()) == 0.0
    assert float(R.udf_head_bwd(sign, dudf, None, 1.3, 7, 4, F64)[:, 1:].abs().max()) == 0.0
    Rm, out0 = torch.randn(7, 3, generator=g), torch.randn(3, generator=g)
    close(R.signed_colsum(sign, Rm, 0.7, out0, F64), out0.double() + 0.7 * (sign.double() @ Rm.double()))
    close(R.signed_colsum(sign, Rm, 0.7, out0, F64, perm=torch.randperm(7, generator=g)), R.signed_colsum(sign, Rm, 0.7, out0, F64))
    # sigmoid head: y = sigmoid(x), loss = (dy + dx) . y + draw . raw
    x = torch.randn(7, 3, generator=g, dtype=F64, requires_grad=True)
    raw = torch.randn(7, 2, generator=g, dtype=F64, requires_grad=True)
    dy, dx, dr = torch.randn(7, 3, generator=g), torch.randn(7, 3, generator=g), torch.randn(7, 2, generator=g)
    y = torch.sigmoid(x)
    ((y * (dy.double() + dx.double())).sum() + (raw * dr.double()).sum()).backward()
    ref = torch.cat([x.grad, raw.grad, torch.zeros(7, 3, dtype=F64)], 1)
    close(R.sigmoid_head_bwd(y.detach(), dy, dx, dr, 2, 8, F64), ref)
    assert float(R.sigmoid_head_bwd(y.detach(), None, None, None, 2, 8, F64).abs().max()) == 0.0


def test_weight_norm_is_torchs_forward_and_backward():
    for out, inp in ((33, 39), (1, 65), (257, 3)):
        L = R.wn_layer(out, inp, 5)
        lin = torch.nn.utils.weight_norm(torch.nn.Linear(inp, out).double())
        with torch.no_grad():
            lin.weight_v.copy_(L["v"].double())
            lin.weight_g.copy_(L["g"].double().reshape(-1, 1))
        x = torch.eye(inp, dtype=F64)
        W = (lin(x) - lin.bias).t()                               # the weight the module applies
        Wp, inv = R.wn_pack(L["v"], L["g"], L["perm"], F64)
        close(Wp[:, L["perm"].long()], W.detach())
        close(inv, 1.0 / L["v"].double().norm(dim=1))
        close(R.wn_pack(L["v"], L["g"], None, F64)[0], W.detach())
        assert torch.equal(R.wn_pack(L["v"], None, None, F32)[0], L["v"])
        dWp = torch.zeros(out, inp)
        dWp[:, L["perm"].long()] = L["dW"]
        (W * L["dW"].double()).sum().backward()
        dv, dg = R.wn_unpack(dWp, L["v"], L["g"], L["perm"], F64)
        close(dv, lin.weight_v.grad)
        close(dg, lin.weight_g.grad.reshape(-1))
        close(R.wn_unpack(dWp, L["v"], None, L["perm"], F64)[0], L["dW"].double())
    assert all(o % 4 and o % 32 for o, _, _, _ in R.WN_TABLE) and len(R.WN_TABLE) >= 4


def test_scalars_and_their_clamps():
    d = torch.tensor([0.3, -1.7, 0.9])
    n_tied = n = 0
    for (var, beta, gamma), hi in [(c, R.BETA_HI) for c in R.SCALAR_CASES] + [(c, 2e6) for c in R.SCALAR_CASES_HI]:
        (s64, r64, d64), (s32, r32, d32) = R.scalars(var, beta, gamma, hi, d, F64), R.scalars(var, beta, gamma, hi, d, F32)
        close(s64, torch.stack([O.inv_s_of({"variance": var.double()}).reshape(()), O.beta_of({"beta": beta.double()}, 1.0 / hi).reshape(()),
                                O.gamma_of({"gamma": gamma.double()}).reshape(())]))
        close(r64, 1.0 / s64[:2])
        assert float(s64.min()) >= 1e-6 and float(s64.max()) <= 1e6 and float(s64[1]) <= hi
        tied = R.scalar_ties(var, beta, gamma, hi)
        for k in range(3):
            n += 1
            n_tied += int(tied[k])
            if not tied[k]:       # fp32 and float64 take the same side of every clamp
                assert (float(d64[k]) == 0.0) == (float(d32[k]) == 0.0)
                e = math.exp(10.0 * float((var, beta, gamma)[k]))
                assert (float(d64[k]) != 0.0) == (1e-6 <= e <= min(1e6, hi if k == 1 else 1e6))
    # A parameter AT a clamp is a tie by construction: whether exp(10 p) passes the clamp there is decided by its last bit.
    # Those are the cases built for it -- 3 + 3 of the six-clamp cases and beta at 1e6 -- and no other: 7 of the 30 derivatives
    # (every VALUE is compared, it is continuous in p).  The 10 % cap of the other rows cannot hold for a case that IS the tie.
    assert (n_tied, n) == (R.SCALAR_TIES, 30)


def test_l1_and_sums_errors():
    for n in R.POINTS:
        c = R.l1_case(n)
        assert float((~c["keep"]).float().mean()) <= R.TIE_CAP
        (s64, g64), (s32, g32) = R.l1_sum(c["pred"], c["gt"], c["d_out"], F64), R.l1_sum(c["pred"], c["gt"], c["d_out"], F32)
        close(s64, (c["pred"].double() - c["gt"].double()).abs().sum())
        eq = (c["pred"] == c["gt"]).reshape(-1)
        assert bool(eq.any()) and float(g64[eq].abs().max()) == 0.0
        assert torch.equal(torch.sign(g64[c["keep"]]), torch.sign(g32[c["keep"]]).double())
        p = torch.randperm(3 * n, generator=torch.Generator().manual_seed(0))
        close(R.l1_sum(c["pred"], c["gt"], c["d_out"], F64, perm=p)[0], s64)
    sums, d = torch.tensor([3.7, 120.0, 0.91, 77.0, 41.5]), torch.tensor([0.7, -1.1, 0.05])
    e, gs = R.sums_errors(sums, 512.0, d, F64)
    close(e, torch.tensor([3.7 / (120.0 + 1e-5), 0.91 / (77.0 + 1e-5), 41.5 / 512.0], dtype=F64), 1e-7)
    h = 1e-6
    for k in range(5):
        sp, sm = sums.double().clone(), sums.double().clone()
        sp[k] += h
        sm[k] -= h
        fd = ((R.sums_errors(sp, 512.0, d, F64)[0] - R.sums_errors(sm, 512.0, d, F64)[0]) * d.double()).sum() / (2 * h)
        assert abs(float(fd) - float(gs[k])) < 1e-7


def test_adam_restatement_is_torch_optim_adam():
    a, b = R.adam_reference(F64), R.adam_torch(F64)
    for x, y in zip(a, b):
        close(x, y, 1e-13)
    # eps decides some updates and is invisible in others: moving it inside the square root moves some elements by more than
    # fp32 resolution and leaves others where they were
    ps0, grads = R.adam_inputs()
    gmax = torch.stack([g[4].abs() for g in grads]).max(0)[0]
    assert float(gmax.min()) < 1e-5 and float(gmax.max()) > 1.0
    small = torch.stack([g[2].abs() for g in grads]).max(0)[0] < 1e-7
    assert bool(small.any()) and not bool(small.all())
    assert sorted(i for grp in R.ADAM_GROUPS for i in grp["idx"]) == list(range(len(R.ADAM_SIZES))) and len(R.ADAM_GROUPS) == 3
    # the fp32 evaluation stays close: e_ref is a rounding figure, not a different algorithm
    r32 = R.adam_reference(F32)
    for x, y in zip(r32, a):
        assert float((x.double() - y).abs().max()) < 1e-5
    # ... and the matrix's bound sees eps: an Adam with eps under the square root misses it on every tensor, by far
    wrong = R.adam_reference(F64, eps_inside=True)
    for n, w, x64, x32 in zip(R.ADAM_SIZES, wrong, a, r32):
        (_, _, err, e_ref, bound, _, _), = R.tiles(w, x64, x32, n, None)
        assert err > 10 * bound, (n, err, e_ref, bound)
