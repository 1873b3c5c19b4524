"""The three MLP engines OFF the shipped conf's network shapes (tests/arch_cases.py): widths that are no multiple of 32, 16
or 4, skip tails at other columns, encodings of 15 ... 93 columns, two to eight layers, with and without weight_norm.

  * engine parity: values, input gradients and every parameter gradient of a random-weighted sum of all outputs (for the
    UDF network including d udf / dx, so the tangent and adjoint sweeps run) against the FLOAT64 oracle, at 97 and 349 points
    (ragged against the 32-point tile; 349 also against a forced 64-point tile), exact fp32 and bf16x3 operands, plus the
    per-layer GEMM path; the backward run twice gives bit-identical gradients;
    bars: values rel < max(1e-4, 3 e_ref32), gradients grel < max(1e-3, 3 e_ref32), e_ref32 = the fp32 oracle's own
    distance from the float64 oracle for that tensor (computed here; at most 1.3e-6 / 6.8e-6, so the bars are 1e-4 / 1e-3);
  * the packed weights bit for bit: W, W^T and every fragment-ordered copy of every layer in four operand modes;
  * the 16-bit mode: 16-bit-tile kernel == fp32-tile kernel bit for bit at these shapes;
  * one whole render and train-step backward with 64-wide networks (feature width 64);
  * the gates: one step outside each, served by the per-layer path or refused before the first launch.

Measured on the MI355X (worst tensor per entry over the 97- and 349-point cases and both tiles; values against the bar
1e-4, gradients -- input and parameter gradients, TRUE relative in the max norm -- against the bar 1e-3):

  entry     exact fp32 chain      bf16x3 chain          per-layer path (bf16x3, 97 points)
            values    gradients   values    gradients   values    gradients
  u64       5.49e-07  1.45e-06    4.77e-07  1.46e-06    4.73e-07  1.49e-06
  u100      1.13e-06  4.95e-06    8.59e-07  2.64e-06    1.23e-06  5.04e-06
  u96       6.90e-07  1.42e-06    4.84e-07  1.77e-06    4.46e-07  1.82e-06
  u250      1.20e-06  5.43e-06    7.97e-07  3.68e-06    1.13e-06  4.87e-06
  u32sq     3.67e-07  1.98e-06    4.38e-07  7.73e-06    3.67e-07  1.07e-06
  u64nw     4.83e-07  1.75e-06    3.75e-07  2.40e-06    3.50e-07  1.69e-06
  c64       5.95e-08  6.66e-07    5.97e-08  4.09e-07    5.41e-08  4.39e-07
  c100      5.70e-08  1.43e-06    6.13e-08  5.28e-07    5.28e-08  4.08e-07
  c29h      5.78e-08  1.14e-06    5.78e-08  9.59e-07    5.65e-08  6.60e-07
  n64       4.24e-08  7.54e-07    6.59e-08  9.03e-07    4.16e-08  4.00e-07
  n96       4.04e-08  7.99e-07    3.44e-08  6.34e-07    2.95e-08  3.56e-07
  u_f100    4.76e-07  1.59e-06    5.42e-07  1.51e-06    5.77e-07  1.69e-06
  c_f100    5.68e-08  8.22e-07    5.86e-08  7.84e-07    5.35e-08  7.04e-07
  g_u288    (gate: per-layer path only)                 7.29e-07  2.21e-06
  g_c33                                                 5.69e-08  3.99e-07
  g_c256v6                                              5.61e-08  7.82e-07
  g_c29                                                 5.60e-08  7.45e-07
  g_n100                                                3.86e-08  3.80e-07

  render, u64 + c64 + n64:  5 rays  worst of 14 outputs 2.32e-06 (vis_prob; bar 1e-4), worst parameter gradient 2.48e-05
                                    (nerf.pts_linears.2.weight; bar 1e-3, the fp32 oracle itself 1.13e-05 from float64)
                            66 rays worst output 9.78e-06 (vis_prob), worst parameter gradient 3.97e-04
                                    (nerf.alpha_linear.weight; bar 3 e_ref32 = 1.2e-3, the fp32 oracle itself 4.07e-04)
  UDF -> colour, F = 100, 97 points: colours 5.39e-08, worst parameter gradient 3.53e-06 (udf.lin2.bias; bar 1e-3)
  refused shapes, forward alone against float64: two skips (per-layer path) 3.45e-07, E = 99 (chain) 5.13e-07

  mixed16, 349 points, 64-point tiles, distance from the exact-fp32 mode (max / max |fp32|; measured, not asserted -- the
  16-bit mode has no accuracy bar below render level); 16-bit-tile kernel == fp32-tile kernel bit for bit in all four:
            values    gradients
  u64       1.25e-03  4.89e-03
  u100      1.83e-03  1.11e-02
  c100      3.45e-04  8.22e-02
  n64       8.73e-04  9.45e-02

u32sq has multires 4 (E = 27): d_hidden = 32 leaves 32 - E columns in front of its skip, so with multires 6 (E = 39) the
module cannot be constructed.  The colour network with d_hidden = 256 and multires_view = 4 (g_c29) is a gate case: the base
head's 32-column tile would end at column 315 of the chain's 288; c29h keeps a 32-wide view head on the chain at the shipped
hidden width.  u_f100 + c_f100 (F = 100, a multiple of 4 but not of 16) exist for the colour net's d CIN entering the UDF adjoint
sweep's 112-column tile load (test_colour_adjoint_enters_the_udf_adjoint_load).
"""
import pytest
import torch

import arch_cases as A
from common import CONF
from oracle import udf_oracle as O

pytestmark = pytest.mark.gpu

VTOL, GTOL = 1e-4, 1e-3
_ON_DEV = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _net(name, dev):
    if name not in _ON_DEV:
        _ON_DEV[name] = A.module(name)[0].to(dev)
    return _ON_DEV[name]


def _kind(name):
    return (A.ALL[name] if name in A.ALL else A.REFUSED[name][0])["kind"]


def _run(name, inp, dev):
    """one forward + backward of the module on the GPU -> (values, gradients) keyed like arch_cases.oracle_run"""
    net, kind = _net(name, dev), _kind(name)
    net.zero_grad()
    D = lambda t: t.to(dev)
    extra = {}
    if kind == "udf":
        F = net.n_feature
        udf, feat, grad = net.evaluate(D(inp["x"]), want_grad=True)
        wy, wg = D(inp["wy"]), D(inp["wg"])
        ((udf * wy[:, 0]).sum() + (feat[:, :F] * wy[:, 1:]).sum() + (grad * wg).sum()).backward()
        vals = dict(udf=udf, feat=feat[:, :F], grad=grad)
    elif kind == "color":
        fd = D(inp["feat"]).detach().requires_grad_(True)
        out = net(D(inp["pts"]), D(inp["nrm"]), D(inp["dirs"]), fd)
        sum((a * D(b)).sum() for a, b in zip(out, inp["w"])).backward()
        vals = dict(color_base=out[0], color=out[1], logits=out[2])
        extra["d_feat"] = fd.grad
    else:
        s, rgb = net(D(inp["pts4"]), D(inp["dirs"]))
        ((s * D(inp["w"][0])).sum() + (rgb * D(inp["w"][1])).sum()).backward()
        vals = dict(sigma=s, rgb=rgb)
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    grads.update(extra)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in vals.items()}, grads


def _against_float64(tag, vals, grads, ref):
    """print the worst figures, then hold every tensor to its bar"""
    ev = {k: (A.rel(vals[k], ref["vals"][k]), max(VTOL, 3.0 * ref["e_vals"][k])) for k in ref["vals"]}
    assert set(grads) == set(ref["grads"]), sorted(set(grads) ^ set(ref["grads"]))
    eg = {k: (A.grel(grads[k], ref["grads"][k]), max(GTOL, 3.0 * ref["e_grads"][k])) for k in ref["grads"]}
    wv = max(ev.items(), key=lambda kv: kv[1][0] / kv[1][1])
    wg = max(eg.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"arch sweep [{tag}]: {len(ev)} value tensors, worst {wv[0]} rel {wv[1][0]:.2e} (bar {wv[1][1]:.1e}); "
          f"{len(eg)} gradient tensors, TRUE relative worst {wg[0]} inf {wg[1][0]:.2e} (bar {wg[1][1]:.1e}; reference fp32 vs "
          f"float64 {ref['e_grads'][wg[0]]:.2e})")
    for k, (e, bar) in ev.items():
        assert e < bar, (tag, "value", k, e, "bar", bar)
    for k, (e, bar) in eg.items():
        assert e < bar, (tag, "gradient", k, e, "bar", bar, "reference fp32 vs float64", ref["e_grads"][k])


class _switches:
    """mlp's module-level switches for one block, restored whatever happens"""

    def __init__(self, precision=None, tile=0, use_chain=True):
        self.precision, self.tile, self.use_chain = precision, tile, use_chain

    def __enter__(self):
        from neuraludf_amd import mlp
        self.old = (mlp.PRECISION, mlp.CHAIN_TILE, mlp.USE_CHAIN)
        if self.precision is not None:
            mlp.set_precision(self.precision)
        mlp.CHAIN_TILE, mlp.USE_CHAIN = self.tile, self.use_chain

    def __exit__(self, *exc):
        from neuraludf_amd import mlp
        mlp.PRECISION, mlp.CHAIN_TILE, mlp.USE_CHAIN = self.old
        return False


def _parity(name, P, tile, prec, use_chain, dev):
    ref = A.reference(name, P)
    eng = _net(name, dev).engine()
    with _switches(prec, tile, use_chain):
        # (a silently narrowed gate would turn the chain cases into per-layer cases)
        assert eng._chain_ok() == (A.ALL[name]["chain"] and use_chain), name
        vals, grads = _run(name, ref["inp"], dev)
        _, again = _run(name, ref["inp"], dev)
    tag = f"{name} P={P} tile={tile or 'auto'} {prec} {'chain' if (use_chain and A.ALL[name]['chain']) else 'layers'}"
    _against_float64(tag, vals, grads, ref)
    # the weight-gradient GEMMs reduce in two deterministic passes (mlp.TN_DETERMINISTIC): the same backward, the same bits
    diff = [k for k in grads if not torch.equal(grads[k], again[k])]
    assert not diff, (tag, "gradients differ between two runs", diff)


# ---------------------------------------------------------------------------------------------------------------------
# 2. engine parity against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("P,tile", [(97, 0), (349, 0), (349, 64)])
@pytest.mark.parametrize("name", list(A.CHAIN))
def test_chain_engines_match_float64(dev, name, P, tile, prec):
    _parity(name, P, tile, prec, True, dev)


@pytest.mark.parametrize("name", list(A.CHAIN))
def test_per_layer_path_matches_float64(dev, name):
    """the cross-check path (mlp.USE_CHAIN = False) at the same shapes"""
    _parity(name, 97, 0, "bf16x3", False, dev)


# ---------------------------------------------------------------------------------------------------------------------
# 3. packed weights, bit for bit: every layer, every fragment kind, three operand modes
# ---------------------------------------------------------------------------------------------------------------------
def _pack_order(eng):
    """the engine's PackedLinears in the order of `_frag_kinds()`"""
    from neuraludf_amd import mlp
    if isinstance(eng, mlp.ColorEngine):
        return eng.base + eng.view
    return eng._all()


def _frag_order(B, group, dev):
    """[K, N] operand -> (zero-padded fragment order [G, NT, 64, group / 2 ... ], same for the K x N mask).  group = 8: the
    fp32 fragments of pack_frag_kernel, out[((g NT + T) 64 + lane) 4 + j] = B[8 g + 4 (lane >> 5) + j][32 T + (lane & 31)];
    group = 16: the 16-bit and split fragments, element (g, T, lane, j) <-> B[16 g + 8 (lane >> 5) + j][32 T + (lane & 31)]"""
    from neuraludf_amd import mlp
    K, N = B.shape
    NT, G = (N + 31) // 32, mlp.k8(K) // group
    out = []
    for src in (B, torch.ones_like(B)):
        ref = torch.zeros(G * group, NT * 32, device=dev)
        ref[:K, :N] = src
        out.append(ref.reshape(G, 2, group // 2, NT, 32).permute(0, 3, 1, 4, 2).reshape(G, NT, 64, group // 2).contiguous())
    return out[0], out[1] > 0


def _bits16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("name", ["u100", "u250", "u64nw", "c100", "n64"])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16x3-six", "mixed16"])
def test_packed_weights_bit_for_bit(dev, prec, name):
    """prec "bf16x3" is the default split (two fp16 planes on every sweep, dtype 4), "bf16x3-six" the same mode with six bf16
    products everywhere (mlp.set_fwd_split("0"): three bf16 planes, dtype 3)."""
    from neuraludf_amd import mlp
    net = _net(name, dev)
    eng = net.engine()
    old_split = mlp.FWD_F16X2
    try:
        if prec == "bf16x3-six":
            mlp.set_fwd_split("0")
        _packed_weights(dev, prec.split("-")[0], name, eng)
    finally:
        mlp.set_fwd_split(old_split)
        eng.invalidate()


def _packed_weights(dev, prec, name, eng):
    from neuraludf_amd import mlp
    with _switches(prec):
        eng.invalidate()
        _run(name, A.inputs(A.ALL[name], 64), dev)       # one forward + gradient + backward packs every copy of the mode
        kinds = eng._frag_kinds()
        layers = _pack_order(eng)
        assert len(kinds) == len(layers)
        seen = set()
        for li, (pl, ks) in enumerate(zip(layers, kinds)):
            # ---- the packed matrices themselves ----
            W, Wt = pl.W, pl.Wt
            assert torch.equal(Wt[:pl.inp, :pl.out], W[:pl.out, :pl.inp].t()), (name, li, "W^T")
            for what, pad in (("W rows", W[pl.out:]), ("W columns", W[:, pl.inp:]), ("W^T rows", Wt[pl.inp:]),
                              ("W^T columns", Wt[:, pl.out:])):
                assert pad.numel() == 0 or float(pad.abs().max()) == 0.0, (name, li, what)
            v = (pl.lin.weight_v if pl.weight_norm else pl.lin.weight).detach().double()
            ref = v
            if pl.weight_norm:
                ref = pl.lin.weight_g.detach().double() * v / v.norm(dim=1, keepdim=True)
            got = W[:pl.out, :pl.inp].double()
            if pl._perm_list is not None:      # packed column perm[i] holds the module's column i
                got = got[:, torch.tensor(pl._perm_list, device=dev)]
            # 32 fp32 ulps per element: a 64-lane tree sum of <= 5 squares per lane, a square root, a reciprocal and two
            # multiplies are ~10 roundings; a wrong row norm or a misplaced column is an O(1) error
            ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=1e-300))) - 23)
            bad = (got - ref).abs() > 32 * ulp
            assert not bool(bad.any()), (name, li, "W vs float64 g v / |v|", float(((got - ref).abs() / ulp).max()), "ulps")
            # ---- every fragment-ordered copy ----
            for kind in ks:
                tr, o0, i0, K, N, dt = mlp._frag_spec(pl, kind)
                # the branch of wn_pack_multi_kernel that writes this copy: transposed slots, row slots (row offset a multiple
                # of 8) or the element-by-element fallback
                seen.add(("transposed" if tr else ("rows" if o0 % 8 == 0 else "elements"), dt, "tail" if K % 16 else "full"))
                B = (Wt[i0:i0 + K, o0:o0 + N] if tr else W[o0:o0 + K, i0:i0 + N]).contiguous()
                assert B.shape == (K, N), (name, li, kind, B.shape)
                f = pl._frags[kind]
                NT = (N + 31) // 32
                tag = (name, prec, li, kind)
                if dt == 0:
                    ref8, _ = _frag_order(B, 8, dev)
                    assert f.numel() == ref8.numel(), tag
                    assert torch.equal(f.view(torch.int32), ref8.reshape(-1).view(torch.int32)), tag
                    continue
                ref16, inside = _frag_order(B, 16, dev)
                G16 = mlp.k8(K) // 16
                if dt in (1, 2):
                    want = ref16.half() if dt == 1 else ref16.bfloat16()
                    got16 = f.view(torch.float16 if dt == 1 else torch.bfloat16)
                    assert got16.numel() == want.numel(), tag
                    assert torch.equal(_bits16(got16), _bits16(want).reshape(-1)), tag
                elif dt == 3:
                    planes = f.view(torch.int16).reshape(G16, NT, 3, 64, 8)
                    w = (planes.to(torch.int32) << 16).view(torch.float32)
                    total = (w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]
                    assert torch.equal(total, ref16), tag
                    assert not bool((planes != 0).any(dim=2)[~inside].any()), tag + ("non-zero outside K x N",)
                else:
                    assert dt == 4
                    planes = f.view(torch.float16).reshape(G16, NT, 2, 64, 8)
                    hi = ref16.half()
                    lo = ((ref16 - hi.float()) * 2048.0).half()
                    assert torch.equal(_bits16(planes[:, :, 0]), _bits16(hi)), tag + ("hi",)
                    assert torch.equal(_bits16(planes[:, :, 1]), _bits16(lo)), tag + ("lo",)
    print(f"packed weights [{name} {prec} split {mlp.FWD_F16X2}]: {len(layers)} layers, {sum(len(k) for k in kinds)} fragment copies; "
          f"(branch, dtype, K tail) combinations {sorted(seen)}")
    # the walk reached what it is there for: every branch of the pack kernel the network has, in the mode's operand types, with
    # a K tail -- a change of `_frag_kinds_build` that drops one of them must not pass unnoticed
    split = 3 if mlp.FWD_F16X2 == "0" else 4
    d_t, d_r = {"fp32": (0, 0), "bf16x3": (split, split), "mixed16": (1, 2)}[prec]
    need = {("transposed", d_t, "tail"), ("rows", d_r, "tail")}
    if name.startswith("u"):           # the head's feature rows start at row 1 of W: bwd_feat goes element by element
        need.add(("elements", d_r, "tail" if name == "u100" else "full"))       # (K = F: 33 / 256 / 64)
    assert need <= seen, (name, prec, sorted(need - seen))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the 16-bit mode at these shapes: the two tile kernels agree bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u64", "u100", "c100", "n64"])
def test_mixed16_tile_kernels_bit_identical(dev, name):
    from neuraludf_amd import _lib
    lib = _lib.lib()
    P = 349
    inp = A.inputs(A.ALL[name], P)
    with _switches("fp32", 64):
        v32, g32 = _run(name, inp, dev)
    old = lib.nudf_set_chain_t16(1)
    try:
        with _switches("mixed16", 64):
            va, ga = _run(name, inp, dev)
            lib.nudf_set_chain_t16(0)
            vb, gb = _run(name, inp, dev)
    finally:
        lib.nudf_set_chain_t16(old)
    a, b, r = dict(va, **ga), dict(vb, **gb), dict(v32, **g32)
    assert set(a) == set(b) == set(r)
    dv = max(A.grel(va[k], v32[k]) for k in va)
    dg = max(A.grel(ga[k], g32[k]) for k in ga)
    print(f"mixed16 [{name} P={P}, 64-point tiles]: {len(a)} tensors; distance from the fp32 mode (max / max |fp32|): values "
          f"{dv:.2e}, gradients {dg:.2e}")
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, [(k, float((a[k].float() - b[k].float()).abs().max())) for k in diff]
    assert all(bool(torch.isfinite(t.float()).all()) for t in a.values())
    # the 16-bit kernels really ran: no value tensor and not every gradient equals the fp32 mode's
    assert not any(torch.equal(va[k], v32[k]) for k in va), [k for k in va if torch.equal(va[k], v32[k])]
    assert any(not torch.equal(ga[k], g32[k]) for k in ga)


# ---------------------------------------------------------------------------------------------------------------------
# 5. one whole render and train-step backward with 64-wide networks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rays", [5, 66])
def test_render_and_backward_off_the_default_shapes(dev, n_rays):
    from neuraludf_amd import synth
    from neuraludf_amd.models import fields
    from neuraludf_amd.models.udf_renderer_blending import UDFRendererBlending
    names = dict(udf="u64", color="c64", nerf="n64")
    assert A.ALL["u64"]["kw"]["d_out"] - 1 == A.ALL["c64"]["kw"]["d_feature"] == 64
    mods = {k: _net(v, dev) for k, v in names.items()}
    mods["var"] = fields.SingleVarianceNetwork(**CONF["var"]).to(dev)
    mods["beta"] = fields.BetaNetwork(**CONF["beta"]).to(dev)
    sds = {k: A.module(v)[1] for k, v in names.items()}
    sds["var"] = {n: t.detach().cpu().clone() for n, t in mods["var"].state_dict().items()}
    sds["beta"] = {n: t.detach().cpu().clone() for n, t in mods["beta"].state_dict().items()}
    kw = dict(n_samples=17, n_importance=0, n_outside=7, up_sample_steps=1)      # fixed samples: no selection ties
    cfg = O.RenderCfg(perturb=0, udf=A.ALL["u64"]["cfg"], color=A.ALL["c64"]["cfg"], nerf=A.ALL["n64"]["cfg"], **kw)
    r = synth.make_rays(synth.make_scene("tiny"), 0, n_rays, seed=1700 + n_rays)
    w = torch.randn(n_rays, 3, generator=torch.Generator().manual_seed(n_rays))

    def oracle(dtype):
        nets = O.Nets(**{k: A.oracle_sd(sd, dtype) for k, sd in sds.items()})
        c = lambda t: t.to(dtype)
        out = O.render(nets, cfg, c(r["rays_o"]), c(r["rays_d"]), c(r["near"]), c(r["far"]))
        (out["color"] * c(w)).sum().backward()
        return out, nets

    ref32, n32 = oracle(torch.float32)
    torch.set_default_dtype(torch.float64)
    try:
        ref64, n64 = oracle(torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    rend = UDFRendererBlending(mods["nerf"], mods["udf"], mods["var"], mods["color"], mods["beta"], perturb=0.0, **kw)
    D = lambda t: t.to(dev)
    assert all(mods[k].engine()._chain_ok() for k in names)
    with torch.no_grad():
        out = rend.render(D(r["rays_o"]), D(r["rays_d"]), D(r["near"]), D(r["far"]), perturb_overwrite=0)
    worst = ("", 0.0)
    errs = {}
    for k in ("z_vals", "udf", "weights", "color", "color_base", "depth", "normals", "weight_sum", "weight_sum_fg_bg",
              "vis_prob", "alpha", "true_cos", "gradient_error", "gradient_error_near_surface"):
        a, b = out[k].detach().cpu().float().reshape(-1), ref32[k].detach().float().reshape(-1)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        errs[k] = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        if errs[k] > worst[1]:
            worst = (k, errs[k])
    print(f"render off the default shapes [{n_rays} rays]: worst of {len(errs)} outputs {worst[0]} {worst[1]:.2e} (bar 1e-4)")
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)
    # the train-step direction: the same render with gradients, (colour * w).sum().backward()
    for m in mods.values():
        m.zero_grad()
    out = rend.render(D(r["rays_o"]), D(r["rays_d"]), D(r["near"]), D(r["far"]), perturb_overwrite=0)
    assert A.rel(out["color"], ref64["color"]) < VTOL
    (out["color"] * D(w)).sum().backward()
    torch.cuda.synchronize()
    res = {}
    for net in names:
        for pn, p in mods[net].named_parameters():
            g64, g32 = getattr(n64, net)[pn].grad, getattr(n32, net)[pn].grad
            assert p.grad is not None and g64 is not None, (net, pn)
            e32 = A.grel(g32, g64)
            res[f"{net}.{pn}"] = (A.grel(p.grad, g64), max(GTOL, 3.0 * e32), e32)
    wk = max(res, key=lambda k: res[k][0] / res[k][1])
    print(f"render backward off the default shapes [{n_rays} rays]: {len(res)} parameter-gradient tensors, TRUE relative worst "
          f"{wk} inf {res[wk][0]:.2e} (bar {res[wk][1]:.1e}; reference fp32 vs float64 {res[wk][2]:.2e})")
    for k, (e, bar, e32) in res.items():
        assert e < bar, (k, e, "bar", bar, "reference fp32 vs float64", e32)


def test_colour_adjoint_enters_the_udf_adjoint_load(dev):
    """UDF network -> colour network in the renderer's layout, F = 100: the colour net's d CIN [P, 128] is the UDF adjoint sweep's
    initial tile, which loads k8(F) = 112 columns of it -- columns 100 .. 111 meet zero weight rows and must be finite zeros.
    Values and every parameter gradient of both networks against the float64 oracle."""
    from neuraludf_amd import mlp
    P, F = 97, 100
    udf, col = _net("u_f100", dev), _net("c_f100", dev)
    ceng = col.engine()
    assert udf.n_feature == ceng.F == F and ceng.cin_ld == 128 and mlp.k8(F) == 112
    iu, ic = A.inputs(A.ALL["u_f100"], P), A.inputs(A.ALL["c_f100"], P)
    x, dirs, w, wg = iu["x"], ic["dirs"], ic["w"], iu["wg"]

    def oracle(dtype):
        c = lambda t: t.detach().to(dtype).clone()
        su, sc = A.oracle_sd(A.module("u_f100")[1], dtype), A.oracle_sd(A.module("c_f100")[1], dtype)
        y = O.udf_forward(su, c(x), A.ALL["u_f100"]["cfg"])
        g = O.udf_gradient(su, c(x), A.ALL["u_f100"]["cfg"], create_graph=True)
        out = O.color_forward(sc, c(x), None, c(dirs), y[:, 1:], A.ALL["c_f100"]["cfg"])
        (sum((a * c(b)).sum() for a, b in zip(out, w)) + (g * c(wg)).sum()).backward()
        grads = {"udf." + n: t.grad for n, t in su.items()}
        grads.update({"color." + n: t.grad for n, t in sc.items()})
        return [o.detach() for o in out], grads

    v64, g64 = oracle(torch.float64)
    v32, g32 = oracle(torch.float32)
    D = lambda t: t.to(dev)
    with _switches("bf16x3"):
        assert udf.engine()._chain_ok() and ceng._chain_ok()
        udf.zero_grad()
        col.zero_grad()
        _, CIN, g = udf.evaluate(D(x), want_grad=True, feat_ld=ceng.cin_ld)
        out = col.evaluate(CIN, D(dirs), 1)
        loss = sum((a * D(b)).sum() for a, b in zip(out, w)) + (g * D(wg)).sum()
        # what torch.empty hands out next is whatever was freed last: leave non-finite values where d CIN will be allocated
        del_me = torch.full((mlp.pad_rows(P), ceng.cin_ld), float("nan"), device=dev)
        del del_me
        loss.backward()
        torch.cuda.synchronize()
    ev = max(A.rel(a, b) for a, b in zip(out, v64))
    res = {}
    for net, mod in (("udf", udf), ("color", col)):
        for n, p in mod.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (net, n)
            k = f"{net}.{n}"
            res[k] = (A.grel(p.grad, g64[k]), max(GTOL, 3.0 * A.grel(g32[k], g64[k])))
    wk = max(res, key=lambda k: res[k][0] / res[k][1])
    print(f"colour adjoint into the UDF adjoint load [F = {F}, P = {P}]: colours worst rel {ev:.2e} (bar {VTOL}); {len(res)} "
          f"parameter-gradient tensors, TRUE relative worst {wk} inf {res[wk][0]:.2e} (bar {res[wk][1]:.1e})")
    assert ev < max(VTOL, 3.0 * max(A.rel(a, b) for a, b in zip(v32, v64)))
    for k, (e, bar) in res.items():
        assert e < bar, (k, e, "bar", bar)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the gates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.GATE))
def test_one_step_outside_a_gate_runs_per_layer(dev, name):
    _parity(name, 97, 0, "bf16x3", True, dev)


@pytest.mark.parametrize("name", list(A.REFUSED))
def test_unserved_shapes_are_refused_before_any_launch(dev, name, monkeypatch):
    from neuraludf_amd import mlp
    from neuraludf_amd._lib import NudfError
    entry, exc = A.REFUSED[name]
    exc = NudfError if exc == "NudfError" else exc
    net = _net(name, dev)
    eng = net.engine()
    assert eng._chain_ok() == entry["chain"]
    x = A.inputs(entry, 97)["x"].to(dev)
    launched = []
    real = mlp.call
    monkeypatch.setattr(mlp, "call", lambda fn, *a: (launched.append(fn), real(fn, *a))[1])
    with pytest.raises(exc):
        net.evaluate(x, want_grad=True)
    assert launched == [], launched
    # the value alone needs neither a second skip's reverse sweep nor the encoding's VJP: it is served
    with torch.no_grad():
        y = net(x)
    assert launched, "the forward did not go through mlp.call"
    ref = O.udf_forward(A.oracle_sd(A.module(name)[1], torch.float64, False), x.cpu().double(), entry["cfg"])
    e = A.rel(y, ref)
    print(f"refused [{name}]: {exc.__name__} before the first launch; forward alone vs float64 {e:.2e} (bar {VTOL})")
    assert e < VTOL
