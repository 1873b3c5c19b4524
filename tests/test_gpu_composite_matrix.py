"""Every instantiation of the composite kernels and of the up-sampler against float64 (tests/composite_ref.py).

Composite.  nudf_composite_fwd / _bwd (the dispatch at the end of csrc/composite.hip) pick, with nc = ceil((S + n_out) / 64)
and NC = nc for nc <= 6, else 8:
    forward   <NC, DIAG>   any of the twelve diagnostic arrays asked for        (diagnostics=True)
              <NC, FULL>   else, S == 64 NC and n_out == 0 and s_nominal >= S   (what training runs)
              <NC, plain>  else
    backward  <NC, FULL>   S == 64 NC and n_out == 0 and s_nominal >= S,  <NC, ragged> else.
Every case below runs forward + backward twice, diagnostics on and off:

    NC  (S, n_out[, s_nominal])                                          diagnostics off: fwd / bwd
    1   (1,0) (2,0) (63,1)                                                <1, plain> / <1, ragged>
        (64,0)                                                            <1, FULL>  / <1, FULL>
    2   (65,0) (128,0,100)                                                <2, plain> / <2, ragged>
        (128,0)                                                           <2, FULL>  / <2, FULL>
    3   (128,9) (100,33)                                                  <3, plain> / <3, ragged>
        (192,0)                                                           <3, FULL>  / <3, FULL>
    4   (250,0) (256,0,192) (250,0,240)                                   <4, plain> / <4, ragged>
        (256,0)                                                           <4, FULL>  / <4, FULL>
    5   (300,7)                                                           <5, plain> / <5, ragged>
        (320,0)                                                           <5, FULL>  / <5, FULL>
    6   (350,20)                                                          <6, plain> / <6, ragged>
        (384,0)                                                           <6, FULL>  / <6, FULL>
    8   (385,0) (352,33) (448,0) (400,33) [nc 7: one dead chunk] (449,0) (479,33) (449,0,400)
                                                                          <8, plain> / <8, ragged>
        (512,0)                                                           <8, FULL>  / <8, FULL>
    diagnostics on: <NC, DIAG> forward and the ragged-or-FULL backward of the same row, for every shape.
(tests/test_composite_ref.py asserts on the CPU that the table reaches all 21 forward and 14 backward instantiations.)
(448,0) is the case that found a bug: the dispatch took S == 64 nc for FULL, and nc = 7 runs <8> -- whose eighth, dead
chunk then counted as live and stored 64 weights (and gradients) past the end of every ray's row.

Bound, per case, run and tensor: err <= min(max(4 e_ref, floor), 1e-3), err = max|a - b| / max|b| against float64 -- per
64-sample chunk for per-sample tensors, per tensor otherwise; e_ref = the same error of the fp32 torch evaluation of the
reference helper on that case; floor 1e-5 for values, 1e-4 for gradients.  `inside` and `flip` must be equal.  Measured
ratios err / max(e_ref, floor / 4): profiles/r08_composite_matrix.txt.

Up-sampler (csrc/upsample.hip: nc = ceil(M / 64); <1> <2> <3> <4>, else <8>; namespace up_exact with
NUDF_UP_NOCONTRACT -- part of the shipped flags -- else up_fast):
    M    64   65   129  192  256  257  320  449  511  512
    <NC> 1    2    3    3    4    8    8    8    8    8
shipped flags (up_exact) at every M, both modes; flags = NUDF_UP_NOCONTRACT alone (up_exact, wave-parallel scans) and
flags = 0 (up_fast) at M = 64, 65, 129, 256, 320, 512 (one M per <NC>, and both ends of <8>).
"""
import math
import os

import pytest
import torch

import composite_ref as R

pytestmark = pytest.mark.gpu

_RATIOS = {}      # (class, nc) -> (ratio, case, run, tensor, err, e_ref)
_UP_ROWS = []


@pytest.fixture(scope="module")
def dev():
    from neuraludf_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    _lib.bind_status(d)                # the composite and up-sampling launches below OR into this word
    _lib.read_status(d, clear=True)
    yield d
    path = os.environ.get("NUDF_MATRIX_REPORT")
    if path:
        _write_report(path)


def _write_report(path):
    with open(path, "w") as f:
        f.write("worst err / max(e_ref, floor / 4) per tensor class and chunk count (bound: 4)\n")
        f.write("%-22s %3s %8s  %s\n" % ("class", "nc", "ratio", "worst: case, run, tensor, err, e_ref"))
        for (cls, nc), (r, case, run, nm, e, er) in sorted(_RATIOS.items()):
            f.write("%-22s %3d %8.3f  %s %s %s err %.2e e_ref %.2e\n" % (cls, nc, r, case, run, nm, e, er))
        f.write("\nup-sampler, per-ray max|dz| against float64: kernel (E_k) and fp32 oracle (E_ref)\n")
        for row in _UP_ROWS:
            f.write(row + "\n")


def _class_of(nm):
    if nm in R.PER_SAMPLE_VALUES:
        return "per-sample values"
    if nm in R.PER_RAY_VALUES:
        return "per-ray values"
    if nm in R.PER_SAMPLE_GRADS:
        return "per-sample gradients"
    return "batch gradients"


def _launch(dev, inp, cfg, diagnostics, colours=True, backward=True, scalar_params=None):
    """one forward (+ backward of the fixed linear functional) through _CompositeFn -> (outputs, gradients) on the host"""
    from neuraludf_amd.models.udf_renderer_blending import _CompositeFn
    D = lambda t: None if t is None else t.to(dev)
    L = lambda t: None if t is None else t.detach().clone().to(dev).requires_grad_(backward)
    lv = dict(udf=L(inp["udf"]), grad=L(inp["grad"]), color=L(inp["color"]) if colours else None,
              color_base=L(inp["color_base"]) if colours else None, bg_sigma=L(inp["bg_sigma"]), bg_color=L(inp["bg_color"]))
    c = dict(s_nominal=cfg["s_nominal"], cos_anneal=cfg["cos_anneal"], flip_saturation=cfg["flip_saturation"],
             use_norm_grad=cfg["use_norm_grad"], sparse_scale=cfg["sparse_scale"], diagnostics=diagnostics,
             alpha_type=cfg["alpha_type"])
    scal = par = None
    if scalar_params is None:
        scal = L(torch.cat([inp["inv_s"], inp["beta"], inp["gamma"]]))
        tail = (scal,)
    else:
        par = [L(p) for p in scalar_params[:3]]
        c["beta_hi"] = float(scalar_params[3])
        tail = (None, par[0], par[1], par[2])
    sd = torch.tensor([inp["sdist"]], device=dev)
    with torch.set_grad_enabled(backward):
        outs = _CompositeFn.apply(c, D(inp["rays_o"]), D(inp["rays_d"]), D(inp["z"]), sd, D(cfg["background_rgb"]),
                                  lv["udf"], lv["grad"], lv["color"], lv["color_base"], D(inp["bg_z"]), lv["bg_sigma"],
                                  lv["bg_color"], *tail)
    names = ["color", "color_base", "weights", "depth", "normals", "wsum", "wsum_all", "sums"]
    o = dict(zip(names, outs[:8]))
    if diagnostics:
        o.update(zip(R.DIAG, outs[8:20]))
    if scalar_params is not None:
        o["scal_out"] = outs[-2]
    grads = {}
    if backward:
        R.functional(o, inp["wts"], lambda t: t.to(dev)).backward()
        G = lambda t: None if t is None else t.grad.detach().cpu()
        grads = dict(d_udf=G(lv["udf"]), d_grad=G(lv["grad"]), d_color=G(lv["color"]), d_color_base=G(lv["color_base"]),
                     d_bg_sigma=G(lv["bg_sigma"]), d_bg_color=G(lv["bg_color"]))
        if scal is not None:
            grads.update(d_inv_s=scal.grad[0:1].cpu(), d_beta=scal.grad[1:2].cpu(), d_gamma=scal.grad[2:3].cpu())
        else:
            grads["d_param"] = torch.cat([p.grad.detach().reshape(1) for p in par]).cpu()
    return {k: v.detach().cpu() for k, v in o.items()}, grads


def _hold(case, run, S, nc, got, ref64, ref32, names, fails):
    """the bound of the module docstring for each named tensor; prints every figure, appends misses to `fails`"""
    for nm in names:
        if ref64.get(nm) is None:
            continue
        a, b, r32 = got[nm], ref64[nm], ref32[nm]
        if nm in R.EXACT:
            if not torch.equal(a.double(), b):
                fails.append("%s %s %s: %d samples differ" % (case, run, nm, int((a.double() != b).sum())))
            continue
        e, er = R.error(nm, a, b, S), R.error(nm, r32, b, S)
        bd = R.bound(nm, er)
        rt = R.ratio(nm, e, er)
        print("%s %-5s %-13s err %.2e e_ref %.2e bound %.1e ratio %.2f" % (case, run, nm, e, er, bd, rt))
        key = (_class_of(nm), nc)
        if key not in _RATIOS or rt > _RATIOS[key][0]:
            _RATIOS[key] = (rt, case, run, nm, e, er)
        if not e <= bd:
            worst = ""
            if nm in R.PER_SAMPLE_VALUES or nm in R.PER_SAMPLE_GRADS:
                off = S if nm in ("d_bg_sigma", "d_bg_color") else 0
                worst = " per chunk: " + " ".join("%d:%.1e" % (k, x) for k, x, _ in R.chunk_errors(a, b, off))
            fails.append("%s %s %s: err %.3e > bound %.1e (e_ref %.2e, ratio %.1f)%s" % (case, run, nm, e, bd, er, rt, worst))


@pytest.mark.parametrize("diagnostics", [True, False], ids=["diag", "train"])
@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_composite_against_float64(dev, idx, diagnostics):
    c = R.CASES[idx]
    inp, cfg, o64, g64, o32, g32 = R.reference(idx)
    bad = R.degenerate(inp, cfg, o64, g64)
    assert not bad, ("degenerate inputs", bad)
    case, run, nc = R.case_id(c), "diag" if diagnostics else "train", R.n_chunks(c["S"], c["n_out"])
    print(case, run, R.instantiation(c["S"], c["n_out"], c["s_nominal"], diagnostics), {k: c[k] for k in
          ("cos_anneal", "use_norm_grad", "alpha_type", "flip_saturation", "background")})
    o, g = _launch(dev, inp, cfg, diagnostics)
    fails = []
    vals = ["weights"] + (R.DIAG if diagnostics else []) + R.PER_RAY_VALUES
    _hold(case, run, c["S"], nc, o, o64, o32, vals, fails)
    _hold(case, run, c["S"], nc, g, g64, g32, R.PER_SAMPLE_GRADS + R.BATCH_GRADS, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("S", [128, 320, 512])
def test_weights_first_form_is_bit_identical(dev, S):
    """color = color_base = None: 'everything but the two colour sums' -- the same weights, depth, normals, both weight
    sums and the five batch sums as the launch with colours, bit for bit (forward only, as rendering runs it)"""
    idx = [i for i, c in enumerate(R.CASES) if (c["S"], c["n_out"], c["s_nominal"]) == (S, 0, S)][0]
    inp, cfg = R.reference(idx)[:2]
    for diagnostics in (False, True):
        full, _ = _launch(dev, inp, cfg, diagnostics, backward=False)
        first, _ = _launch(dev, inp, cfg, diagnostics, colours=False, backward=False)
        for nm in ["weights", "depth", "normals", "wsum", "wsum_all", "sums"] + (R.DIAG if diagnostics else []):
            assert torch.equal(full[nm], first[nm]), (nm, diagnostics)


def test_two_stage_reductions_second_iteration(dev):
    """4101 rays = 1026 workgroups: the b += 1024 loop of partial_sums_body runs a second trip, for the five forward sums
    (partial_sums_kernel, K = 5), for d inv_s / d beta / d gamma (K = 3) and, with the scalars formed from the three
    parameters, for partial_sums_scalars_kernel (o_d_param).  Deterministic: two runs agree bit for bit."""
    N = 4101
    assert (N + 3) // 4 > 1024
    inp = R.make_case(64, 0, 9000, n_rays=N)
    cfg = dict(s_nominal=64, cos_anneal=0.6, flip_saturation=0.9, use_norm_grad=False, alpha_type=0, sparse_scale=25000.0,
               background_rgb=inp["background_rgb"])
    assert min(R.margins(inp).values()) >= R.MARGIN, "degenerate inputs"
    o64, g64 = R.evaluate(inp, cfg, torch.float64)
    o32, g32 = R.evaluate(inp, cfg, torch.float32)
    bad = R.degenerate(inp, cfg, o64, g64)
    assert not bad, ("degenerate inputs", bad)
    fails = []
    o, g = _launch(dev, inp, cfg, False)
    o2, g2 = _launch(dev, inp, cfg, False)
    assert torch.equal(o["sums"], o2["sums"])
    for nm in R.BATCH_GRADS:
        assert torch.equal(g[nm], g2[nm]), nm
    _hold("N4101_S64", "scal", 64, 1, o, o64, o32, ["weights"] + R.PER_RAY_VALUES, fails)
    _hold("N4101_S64", "scal", 64, 1, g, g64, g32, R.PER_SAMPLE_GRADS + R.BATCH_GRADS, fails)
    # the three scalars formed inside the launches from the 1-element parameters; their gradients through exp and clips
    par = (torch.tensor([math.log(30.0) / 10]), torch.tensor([math.log(60.0) / 10]), torch.tensor([math.log(20.0) / 10]),
           1.0 / 0.00005)
    p64, pg64 = R.evaluate(inp, cfg, torch.float64, scalar_params=par)
    p32, pg32 = R.evaluate(inp, cfg, torch.float32, scalar_params=par)
    po, pg = _launch(dev, inp, cfg, False, scalar_params=par)
    po2, pg2 = _launch(dev, inp, cfg, False, scalar_params=par)
    assert torch.equal(po["sums"], po2["sums"]) and torch.equal(pg["d_param"], pg2["d_param"])
    _hold("N4101_S64", "param", 64, 1, po, p64, p32, ["weights", "sums", "color"], fails)
    for k, nm in enumerate(("variance", "beta", "gamma")):      # per scalar: one tensor each, as d_inv_s / d_beta / d_gamma
        _hold("N4101_S64", "param", 64, 1, {"d_" + nm: pg["d_param"][k:k + 1]}, {"d_" + nm: pg64["d_param"][k:k + 1]},
              {"d_" + nm: pg32["d_param"][k:k + 1]}, ["d_" + nm], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# up-sampler
# ------------------------------------------------------------------------------------------------------------------ #
_ALT_M = [64, 65, 129, 256, 320, 512]
SHIPPED = None


def _renderer():
    from neuraludf_amd.models.udf_renderer_blending import UDFRendererBlending
    return UDFRendererBlending(None, None, None, None, None, n_samples=64, n_importance=0, n_outside=0, up_sample_steps=1,
                               perturb=0.0)


def _upsample(dev, inp, mode, K, inv_s, beta, gamma, flags=SHIPPED):
    from neuraludf_amd.models import udf_renderer_blending as urb
    rend = _renderer()
    old = urb.UPSAMPLE_FLAGS
    if flags is not SHIPPED:
        urb.UPSAMPLE_FLAGS = flags
    try:
        with torch.no_grad():
            z_new, pts = rend._upsample(inp["rays_o"].to(dev), inp["rays_d"].to(dev), inp["z"].to(dev), inp["udf"].to(dev),
                                        torch.tensor([inp["sdist"]], device=dev), K, mode, inv_s, beta, gamma)
    finally:
        urb.UPSAMPLE_FLAGS = old
    z_new, pts = z_new.cpu(), pts.cpu().reshape(inp["N"], K, 3)
    assert torch.allclose(pts, inp["rays_o"][:, None] + inp["rays_d"][:, None] * z_new[..., None], rtol=0, atol=1e-5)
    return z_new


def _variants(M):
    v = [("shipped", SHIPPED)]
    if M in _ALT_M:
        v += [("nocontract", 1024), ("contracted", 0)]
    return v


def test_upsample_no_occ_aware_against_float64(dev):
    """mode 1 is well conditioned (the fp32 oracle sits within ~5e-7 of float64 on these inputs): per ray-round
    max|dz| <= 1e-5 against float64, at most 1 % of the ray-rounds over it (a quantile on a bin edge), the median of every
    round under it.  Pins the prefix-sum carries, the LDS CDF and the binary search of every <NC>."""
    for name in ("shipped", "nocontract", "contracted"):
        n_rounds = n_bad = 0
        for M in R.UP_M:
            flags = dict(_variants(M)).get(name, "skip")
            if flags == "skip":
                continue
            for (K, inv_s, beta, gamma) in R.UP_SETTINGS:
                chunks = set()
                for late in (False, True):
                    inp = R.make_upsample_case(M, late)
                    z64 = R.oracle_upsample(inp, 1, K, inv_s, beta, gamma, torch.float64)
                    z32 = R.oracle_upsample(inp, 1, K, inv_s, beta, gamma, torch.float32)
                    chunks |= set(R.quantile_chunks(inp, z64))
                    zk = _upsample(dev, inp, 1, K, inv_s, beta, gamma, flags)
                    ek = (zk.double() - z64).abs().max(dim=1)[0]
                    er = (z32.double() - z64).abs().max(dim=1)[0]
                    row = "mode 1 %-10s M %3d K %2d %s  E_k median %.1e max %.1e  E_ref median %.1e max %.1e" % (
                        name, M, K, "late" if late else "std ", ek.median(), ek.max(), er.median(), er.max())
                    print(row)
                    if K == 16:                 # (the report keeps the 16-quantile rounds; K = 1 is printed only)
                        _UP_ROWS.append(row)
                    assert float(er.max()) <= 1e-6, "degenerate inputs: the fp32 oracle itself is off"
                    assert float(ek.median()) <= 1e-5, (name, M, K, late, float(ek.median()))
                    n_rounds += inp["N"]
                    n_bad += int((ek > 1e-5).sum())
                if K == 16 and M >= 129:
                    need = set(range(1, R.last_section_chunk(M) + 1))
                    assert need <= chunks, ("degenerate inputs: no new sample in chunks", sorted(need - chunks), M)
        assert n_bad <= n_rounds // 100, (name, n_bad, n_rounds)


@pytest.mark.parametrize("M", R.UP_M)
def test_upsample_unbias_against_float64(dev, M):
    """mode 0 is not well conditioned on long rays (the fp32 oracle itself drifts 1e-4 ... 6e-4 off float64 for M >= 257),
    so the bound is relative to that drift: median(E_k) <= 4 median(E_ref) + 1e-6, p90(E_k) <= 4 p90(E_ref) + 1e-5, per-ray
    errors against float64.  A wrong carry moves the new samples by whole bins (>= 4e-3 at M = 512)."""
    fails = []
    inp = R.make_upsample_case(M)
    for (K, inv_s, beta, gamma) in R.UP_SETTINGS:
        z64 = R.oracle_upsample(inp, 0, K, inv_s, beta, gamma, torch.float64)
        z32 = R.oracle_upsample(inp, 0, K, inv_s, beta, gamma, torch.float32)
        if K == 16 and M >= 129:
            # (the last chunk's sections lie behind every surface of these inputs: z_s <= 2.2, z up to 2.6; their weights
            # enter through the normalisation only -- mode 1 above puts new samples into them)
            need = set(range(1, R.last_section_chunk(M)))
            got = set(R.quantile_chunks(inp, z64))
            assert need <= got, ("degenerate inputs: no new sample in chunks", sorted(need - got))
        er = (z32.double() - z64).abs().max(dim=1)[0]
        for name, flags in _variants(M):
            zk = _upsample(dev, inp, 0, K, inv_s, beta, gamma, flags)
            ek = (zk.double() - z64).abs().max(dim=1)[0]
            med, p90 = float(ek.median()), float(ek.quantile(0.9))
            bm, b9 = 4 * float(er.median()) + 1e-6, 4 * float(er.quantile(0.9)) + 1e-5
            _UP_ROWS.append("mode 0 %-10s M %3d K %2d       E_k median %.1e p90 %.1e  E_ref median %.1e p90 %.1e" % (
                name, M, K, med, p90, float(er.median()), float(er.quantile(0.9))))
            print(_UP_ROWS[-1])
            if not med <= bm:
                fails.append("%s M %d K %d: median %.2e > %.2e" % (name, M, K, med, bm))
            if not p90 <= b9:
                fails.append("%s M %d K %d: p90 %.2e > %.2e" % (name, M, K, p90, b9))
    assert not fails, "\n".join(fails)


def test_status_word_is_zero_after_the_module(dev):
    """none of the launches above reported a non-finite ray, scalar or sample"""
    from neuraludf_amd import _lib
    assert _lib.read_status(dev) == 0
