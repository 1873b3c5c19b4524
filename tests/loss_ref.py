"""The loss kernels (ssim_patch_kernel and patch_metric_kernel<1|2|3> of csrc/blend.hip; color_loss_fwd / _sums / _finish /
_bwd, step_loss_fwd / _bwd and blend_loss_prepare / _fwd / _bwd of csrc/rays_embed.hip) as plain torch functions of a dtype,
the generators of the inputs the loss matrix runs on and the floors of its one-element rows.  No GPU in here.

Every function is restated from the oracle (oracle/udf_oracle.py: pixel_l1, ssim_window, ssim_patch_error, ncc_patch,
patch_error, patch_loss, color_loss) and from the runner's expressions the kernels' comments cite (the patch-mask algebra,
the masked means of the composite sums, the weighted total) -- never from the kernels -- and evaluated twice on the same
fp32-drawn inputs: in float64 (the reference) and in float32 (`e_ref`).  Gradients come from autograd on those expressions.
tests/test_loss_ref.py pins the restatements to the oracle and to finite differences.

Bound: layer_ref.hold, err <= min(max(FACTOR e_ref, floor), CAP max|ref|) per tile of 64 rays.  A loss scalar is ONE element
and a sum taken in an order that is not torch's: its e_ref is the worst of the fp32 evaluation and N_PERM more with the
operands permuted, and it carries a floor of (roundings between the reduced sums and the output) x 2^-24 x the value -- the
form of layer_ref.quotient_floor; each count is explained where it is set (ROUNDINGS).  Per-ray outputs of a launch of at
most 32 elements carry floors of the same kind where a row needs one (the L1 / SSD patch errors, the k rows).

Weights are rounded to fp32 before either precision sees them, as the kernels receive them; the float64 side then forms
every product and sum in float64."""
import functools

import torch

from composite_ref import CAP, FACTOR, MARGIN
from layer_ref import F32, F64, POINTS, TIE_CAP, hold, quotient_floor, tiles
from oracle import udf_oracle as O

__all__ = ["CAP", "FACTOR", "MARGIN", "TIE_CAP", "hold", "tiles", "quotient_floor"]

HALF_ULP = 2.0 ** -24
N_PERM = 6
RAYS = list(POINTS) + [341, 342]          # 3 x 341 = 1023, 3 x 342 = 1026: either side of the 1024-thread stride
MASKS = ["none", "ones", "zeros", "one", "random"]

# index of the weights in the device vector (include/nudf.h NUDF_LW_*)
LW_BASE, LW_COLOR, LW_PIXEL, LW_PATCH, LW_IGR, LW_IGR_NS, LW_SPARSE, LW_MASK, LW_SUM, LW_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16


def f32(x):
    """the fp32 number a by-value float argument or a device vector entry holds, as a Python float"""
    return float(torch.tensor(float(x), dtype=F32))


def _w(base, color, pixel, patch, igr, igr_ns, sparse):
    return dict(base=f32(base), color=f32(color), pixel=f32(pixel), patch=f32(patch), igr=f32(igr), igr_ns=f32(igr_ns),
                sparse=f32(sparse))


# the shipped colour weights with the regulariser weights (igr, igr_ns, sparse) = (0.1, 0.05, 0.01); one set without the
# pixel term; GARBAGE: what the by-value arguments hold when the device vector must win
WEIGHTS = dict(shipped=_w(1.0, 1.0, 0.5, 0.1, 0.1, 0.05, 0.01), no_pixel=_w(1.0, 1.0, 0.0, 0.1, 0.1, 0.05, 0.01),
               uneven=_w(0.7, 1.3, 0.25, 0.2, 0.3, 0.0, 0.02))
GARBAGE = _w(123.0, -7.0, 55.0, 9.0, -3.0, 17.0, 1e3)


def w_dev_vector(w):
    """the device weight vector of NUDF_LW_COUNT floats; COLOR_SUM formed by the host in double, the unused entries NaN"""
    v = torch.full((LW_COUNT,), float("nan"))
    for i, k in ((LW_BASE, "base"), (LW_COLOR, "color"), (LW_PIXEL, "pixel"), (LW_PATCH, "patch"), (LW_IGR, "igr"),
                 (LW_IGR_NS, "igr_ns"), (LW_SPARSE, "sparse")):
        v[i] = w[k]
    v[LW_MASK] = 0.0
    v[LW_SUM] = w["base"] + w["color"] + w["pixel"]
    return v


# ------------------------------------------------------------------------------------------------------------------ #
# floors of the one-element rows: roundings between the reduced sums and the output, 2^-24 of the value each
# ------------------------------------------------------------------------------------------------------------------ #
# Every count opens with SUM = 2, the reduced sum's own last ulp: an fp32 sum of n terms in an order of its own ends one ulp
# (2 x 2^-24) from the nearest fp32 number as often as not, and the handful of permuted fp32 evaluations behind e_ref may all have
# landed ON the nearest.  An integer sum (a mask count, k, the kept count) is exact in any order: 0.
SUM = 2
ROUNDINGS = dict(
    exact=0,
    sum=SUM,
    den=2,             # the constant 1e-4 as an fp32 number, the sum count + 1e-4 (the count itself is exact)
    L=SUM + 3,         # den's two and the quotient sum / den (no mask: den = n exact, the bound only gets looser)
    cl=SUM + 8,        # L's three, the product L w, the sum of the two products, the two sums of w_b + w_c + w_px, the quotient
    reg=SUM + 4,       # s / (t + 1e-5), s / n_rays: layer_ref.quotient_floor's four (used as quotient_floor x (SUM + 4) / 4)
    total=SUM + 12,    # the longest term (cl's eight, or a regulariser's four and its product with a weight) and the three sums;
                       # every term is >= 0 on these inputs, so the relative errors do not amplify
    k_l1=9,            # (g w / W + d) / den: product, W's two sums, quotient, sum, den's two, quotient; the product with +-1 exact
    d_sums=8,          # d / (t + 1e-5)^2 s: the g w product, the sum with d_extra, t + 1e-5 (two), its square, the product
                       # with s, the quotient, the sign
    Lpatch=SUM + 1,    # the quotient of the two reduced sums
    blend_L=SUM + 1,   # Lb, Lc = sum / (3 N)
    blend_cl=SUM + 10, # L (three), the product, two sums, w_sum rounded by the host, the quotient, Lpatch w (the product), the sum
    blend_total=SUM + 14,
    blend_k=5,         # g w / w_sum / den: three operations and den's two
    d_err=3,           # g w keep / count
)


def rfloor(name, value):
    if name == "reg":
        return quotient_floor(value) * ROUNDINGS["reg"] / 4.0
    return ROUNDINGS[name] * HALF_ULP * abs(float(value))


# ------------------------------------------------------------------------------------------------------------------ #
# the patch errors (loss/loss.py:66-73, loss/patch_metric.py)
# ------------------------------------------------------------------------------------------------------------------ #
KINDS = {"ssim": 0, "l1": 1, "ssd": 2, "ncc": 3}
HPS = [1, 3, 4, 5]                          # Npx = 9, 49, 81 (a partly filled second pass of the 64 lanes), 121
PATCH_RAYS = [1, 3, 4, 5, 6, 255, 257]           # 6: the smallest launch that holds all six content classes
# ray r is of class CLASSES[r % 6].  The order decides what the launches of 1, 3, 4 and 5 rays hold.  A flat bright patch has an
# SSIM error of ~3e-5 that NO fp32 evaluation of E[x^2] - mu^2 knows below ~2e-4 (the oracle's own included), so it can be
# held only in a tile whose largest reference is ~0.3 or more (CAP): the classes with the largest errors come first.  Ray 256,
# the one-ray last tile of N = 257, is of class 4 (half): a near-equal patch alone has an error of ~6e-6, under what fp32 resolves.
CLASSES = ["flat_channel", "random", "flat", "equal", "half", "near_equal"]


def npx_of(hps):
    return (2 * hps + 1) ** 2


@functools.lru_cache(maxsize=None)
def window(hps):
    """the fp32 Gaussian window: an input, cast by the float64 side, not recomputed there"""
    return O.ssim_window(hps).float().contiguous()


def _weighted_sums(p, g, w):
    return (p * w).sum(1), (g * w).sum(1), (p * p * w).sum(1), (g * g * w).sum(1), (p * g * w).sum(1)


def _ssim_of_sums(m1, m2, e11, e22, e12):
    s1, s2, s12 = e11 - m1 ** 2, e22 - m2 ** 2, e12 - m1 * m2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    val = 1 - ((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 ** 2 + m2 ** 2 + c1) * (s1 + s2 + c2))
    return val.sum(-1) / 2


def patch_error(pred, gt, win, kind, dtype):
    """pred, gt [N,Npx,3], win [Npx] -> [N]: O.patch_error with the window as an argument"""
    p, g = pred.to(dtype), gt.to(dtype)
    if kind == "l1":
        return (p - g).abs().mean(-1).sum(-1)
    if kind == "ssd":
        return ((p - g) ** 2).mean(-1).sum(-1)
    w = win.to(dtype)[None, :, None]
    if kind == "ssim":
        return _ssim_of_sums(*_weighted_sums(p, g, w))
    mu1, mu2 = (p * w).sum(1), (g * w).sum(1)
    sigma1 = torch.sqrt((p * p * w).sum(1) - mu1 ** 2 + 1e-4)
    sigma2 = torch.sqrt((g * g * w).sum(1) - mu2 ** 2 + 1e-4)
    pn = (p - mu1[:, None]) / (sigma1[:, None] + 1e-8)
    gn = (g - mu2[:, None]) / (sigma2[:, None] + 1e-8)
    return 1 - (pn * gn * w).sum(1).mean(-1)


def patch_error_vjp(pred, gt, win, kind, d_out, dtype, perm=None):
    """-> err [N], d_pred [N,Npx,3] = d (sum err d_out) / d pred.  perm: the patch pixels in another order"""
    if perm is not None:
        pred, gt, win = pred[:, perm], gt[:, perm], win[perm]
    p = pred.to(dtype).clone().requires_grad_(True)
    err = patch_error(p, gt, win, kind, dtype)
    (err * d_out.to(dtype)).sum().backward()
    grad = p.grad
    if perm is not None:
        back = torch.empty_like(perm)
        back[perm] = torch.arange(len(perm))
        grad = grad[:, back]
    return err.detach(), grad


def patch_floor(err64, kind):
    """the floor of err [N], counting in tiles of at most 32 rays only (a launch of N <= 6 rays, the one-ray last tile of N = 257).
    L1 / SSD: the sum over the patch is an fp32 sum of 3 Npx non-negative terms, not known below one ulp (2^-23) of its value
    whatever the order, and its scaling by 1 / 3 rounds the result once more: 2 x 2^-23 |err|.  SSIM, NCC and every gradient:
    none -- e_ref with the patch pixels permuted alone."""
    return 4.0 * HALF_ULP * err64.abs() if kind in ("l1", "ssd") else 0.0


@functools.lru_cache(maxsize=None)
def patch_case(hps, N):
    """pred, gt [N,Npx,3] (ray r is of content class CLASSES[r % 6], so that every launch of N >= 6 rays holds all six and
    the smaller ones the first N), d_out [N] with both signs and exact zeros in a third of the rays, `l1_keep` [N,Npx,3]:
    the elements whose sign(pred - gt) is no tie"""
    npx = npx_of(hps)
    g = torch.Generator().manual_seed(1000 * hps + N)
    R = lambda *s: torch.rand(*s, generator=g)
    G = lambda *s: torch.randn(*s, generator=g)
    pred, gt = torch.empty(N, npx, 3), torch.empty(N, npx, 3)
    for r in range(N):
        cls = CLASSES[r % 6]
        if cls == "random":
            p = R(npx, 3)
            q = (p + 0.1 * G(npx, 3)).clamp(0.0, 1.0)
        elif cls == "near_equal":
            p = R(npx, 3)
            q = p + 1e-3 * G(npx, 3)
        elif cls == "flat":
            # dark in ray 2, bright in ray 8, ...: the launches of 3 to 5 rays hold the dark one.  A bright flat patch leaves
            # sigma^2 = E[x^2] - mu^2 + 1e-4 (NCC) known to 1e-7 / 1e-4 in fp32, the oracle's own evaluation included, and its
            # gradient to 1e-3 of itself: that meets CAP only in a tile with larger gradients beside it (every 64-ray tile)
            col = torch.full((1, 3), 0.02 if (r // 6) % 2 == 0 else 0.9) + 0.01 * R(1, 3)
            p, q = col + 1e-4 * G(npx, 3), col + 1e-4 * G(npx, 3)
        elif cls == "equal":
            p = R(npx, 3)
            q = p.clone()
        elif cls == "half":
            p = torch.zeros(npx, 3)
            p[npx // 2:] = 1.0
            q = p.clone()
            q[torch.randperm(npx, generator=g)[:max(1, npx // 8)]] = 0.5       # (a target equal everywhere would be the class `equal`)
        else:
            p, q = R(npx, 3), R(npx, 3)
            p[:, 1], q[:, 1] = 0.37, 0.37
        pred[r], gt[r] = p, q
    d_out = G(N)
    zero = torch.tensor([(7 * r + r // 6) % 3 == 1 for r in range(N)])
    d_out[zero] = 0.0
    d = pred.double() - gt.double()
    return dict(hps=hps, N=N, npx=npx, pred=pred, gt=gt, win=window(hps), d_out=d_out, zero=zero,
                l1_keep=(d == 0) | (d.abs() > MARGIN))


@functools.lru_cache(maxsize=None)
def patch_rows(kind, hps, N):
    """-> {output: spec} of one patch launch (spec: see `spec`)"""
    c = patch_case(hps, N)
    a = (c["pred"], c["gt"], c["win"], kind, c["d_out"])
    e64, g64 = patch_error_vjp(*a, F64)
    e32, g32 = patch_error_vjp(*a, F32)
    g = torch.Generator().manual_seed(hps + N)
    extra = [patch_error_vjp(*a, F32, perm=torch.randperm(c["npx"], generator=g)) for _ in range(N_PERM)]
    w = c["npx"] * 3
    keep = c["l1_keep"].reshape(-1) if kind == "l1" else None
    return dict(err=spec(e64, e32, [e[0] for e in extra], 64, patch_floor(e64, kind)),
                d_pred=spec(g64.reshape(-1), g32.reshape(-1), [e[1].reshape(-1) for e in extra], 64 * w, 0.0, keep))


def spec(r64, r32, extra=(), tr=64, floor=0.0, keep=None, one_draw=False):
    """one output of a launch: the float64 reference, the fp32 evaluation, further fp32 evaluations with the operands
    permuted, the tile's rows, the floor and the rows kept.  The floor counts in tiles of at most 32 elements only -- unless
    the whole row is ONE number times a pattern of -1 / 0 / 1 (one_draw: the L1 gradients k sign(pred - gt), d_err = k keep),
    whose e_ref is a single draw however many elements carry it"""
    return dict(r64=r64, r32=r32, extra=list(extra), tr=tr, floor=floor, keep=keep, one_draw=one_draw)


def hold_rows(case, specs, got, rows_out, fails):
    """layer_ref.hold for every output of `specs` that `got` has"""
    for name, s in specs.items():
        if name in got and not name.startswith("_") and name not in specs.get("_nan", ()):
            hold(case, name, got[name], s["r64"], s["r32"], s["tr"], None, rows_out, fails, floor=s["floor"], keep=s["keep"],
                 e_ref_extra=s["extra"], floor_all=s["one_draw"])


def reference_holds(case, specs, rows_out, fails):
    """the fp32 restatement itself against the bound that the other fp32 evaluations and the floor give: the reference alone
    must stay inside its bar.  (An output without permuted evaluations is compared with itself: only the cap can fail.)"""
    for name, s in specs.items():
        if name.startswith("_") or name in specs.get("_nan", ()):
            continue
        for ev in [s["r32"]] + s["extra"]:                 # every fp32 evaluation on its own is inside the cap
            for r0, c0, err, _, _, mx, _ in tiles(ev, s["r64"], ev, s["tr"], None, 0.0, s["keep"]):
                if not err <= CAP * mx:
                    fails.append("%s %s tile %d: an fp32 evaluation is off by %.3e > CAP max|ref| = %.3e" % (case, name, r0, err, CAP * mx))
        others = s["extra"] if s["extra"] else [s["r32"]]
        hold(case, name, s["r32"], s["r64"], others[0], s["tr"], None, rows_out, fails, floor=s["floor"], keep=s["keep"],
             e_ref_extra=others[1:], floor_all=s["one_draw"])


# ------------------------------------------------------------------------------------------------------------------ #
# ColorLoss with its two L1 terms (loss/loss.py:105-133, 21-44)
# ------------------------------------------------------------------------------------------------------------------ #
def _l1(pred, gt, mask):
    """O.pixel_l1: the mask only enters the denominator"""
    e = (pred - gt).abs()
    if mask is not None:
        return e.sum() / (mask.sum() + 1e-4)
    return e.mean()


def color_loss(cb, c, gt, mask, w, dtype):
    """-> (total, Lb, Lc, den); den = sum(mask) + 1e-4, or the element count"""
    T = lambda t: None if t is None else t.to(dtype)
    cb, c, gt, mask = T(cb), T(c), T(gt), T(mask)
    Lb, Lc = _l1(cb, gt, mask), _l1(c, gt, mask)
    total = (Lb * w["base"] + Lc * w["color"]) / (w["base"] + w["color"] + w["pixel"])
    den = (mask.sum() + 1e-4) if mask is not None else torch.tensor(float(gt.numel()), dtype=dtype)
    return total, Lb, Lc, den


def color_loss_vjp(cb, c, gt, mask, w, d, dtype):
    """upstream d = (d0, d1, d2) for (total, Lb, Lc) -> (d_cb, d_c)"""
    a, b = cb.to(dtype).clone().requires_grad_(True), c.to(dtype).clone().requires_grad_(True)
    total, Lb, Lc, _ = color_loss(a, b, gt, mask, w, dtype)
    (total * d[0] + Lb * d[1] + Lc * d[2]).backward()
    return a.grad, b.grad


def color_sums(cb, c, gt, mask, dtype):
    """the sharded form's local sums [sum|cb - gt|, sum|c - gt|, sum(mask) or the element count]"""
    T = lambda t: None if t is None else t.to(dtype)
    cb, c, gt, mask = T(cb), T(c), T(gt), T(mask)
    D = mask.sum() if mask is not None else torch.tensor(float(gt.numel()), dtype=dtype)
    return torch.stack([(cb - gt).abs().sum(), (c - gt).abs().sum(), D])


def color_finish(sums, has_mask, w, dtype):
    s = sums.to(dtype)
    den = s[2] + 1e-4 if has_mask else s[2]
    Lb, Lc = s[0] / den, s[1] / den
    return (Lb * w["base"] + Lc * w["color"]) / (w["base"] + w["color"] + w["pixel"]), Lb, Lc, den


def _permute_elements(ts, perm):
    return [t.reshape(-1)[perm].reshape(t.shape) for t in ts]


@functools.lru_cache(maxsize=None)
def color_case(N, third=False):
    """cb, c[, pix], gt [N,3] uniform with every seventh element of each prediction equal to the target (exact zeros);
    keep_*: the elements whose sign(pred - gt) is no tie (0 < |pred - gt| < MARGIN left out)"""
    g = torch.Generator().manual_seed(4000 + N + (500000 if third else 0))
    gt = torch.rand(N, 3, generator=g)
    out = dict(N=N, gt=gt)
    for i, nm in enumerate(("cb", "c", "pix") if third else ("cb", "c")):
        p = torch.rand(N, 3, generator=g)
        p.reshape(-1)[i::7] = gt.reshape(-1)[i::7]
        d = (p.double() - gt.double()).reshape(-1)
        out[nm], out["keep_" + nm] = p, (d == 0) | (d.abs() > MARGIN)
    return out


@functools.lru_cache(maxsize=None)
def mask_case(N, kind):
    """the pixel mask [N,1] of the colour loss (n_mask = N while n = 3 N), or None"""
    g = torch.Generator().manual_seed(6000 + N)
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(N, 1)
    m = torch.zeros(N, 1)
    if kind == "one":
        m[int(torch.randint(0, N, (1,), generator=g))] = 1.0
    if kind == "random":
        m = (torch.rand(N, 1, generator=g) < 0.6).float()
    return m


def mask_count(N, kind):
    m = mask_case(N, kind)
    return None if m is None else int(m.sum())


D_COLOR = [(0.37, 0.0, 0.0), (0.9, -0.4, 0.25), (0.0, 0.0, -1.3)]       # upstream (total, Lb, Lc); any may be zero


def _k_spec(k64, k32, keep, mag, name):
    """a gradient row k sign(pred - gt) [N,3] flattened: tiles of 64 rays; the floor of k for the launches of <= 32 elements"""
    return spec(k64.reshape(-1), k32.reshape(-1), (), 64 * 3, rfloor(name, mag), keep, one_draw=True)


@functools.lru_cache(maxsize=None)
def color_rows(N, mkind, wname, di=0):
    """-> {output: spec} of color_loss_fwd (total, Lb, Lc, den), of its sums and of color_loss_bwd with upstream D_COLOR[di]"""
    c, mask, w, d = color_case(N), mask_case(N, mkind), WEIGHTS[wname], D_COLOR[di]
    a = (c["cb"], c["c"], c["gt"], mask, w)
    r64, r32 = color_loss(*a, F64), color_loss(*a, F32)
    g = torch.Generator().manual_seed(N)
    extra, sums_extra = [], []
    for _ in range(N_PERM):
        pc = _permute_elements((c["cb"], c["c"], c["gt"]), torch.randperm(3 * N, generator=g))
        pm = None if mask is None else mask[torch.randperm(N, generator=g)]
        extra.append(color_loss(*pc, pm, w, F32))
        sums_extra.append(color_sums(*pc, pm, F32))
    out = {}
    for i, (nm, fl) in enumerate((("total", "cl"), ("Lb", "L"), ("Lc", "L"), ("den", "den"))):
        out[nm] = spec(r64[i], r32[i], [e[i] for e in extra], 1, rfloor(fl, r64[i]))
    s64, s32 = color_sums(*a[:4], F64), color_sums(*a[:4], F32)
    for i in range(3):
        out["sums%d" % i] = spec(s64[i], s32[i], [e[i] for e in sums_extra], 1, rfloor("sum" if i < 2 else "exact", s64[i]))
    g64, g32 = color_loss_vjp(*a, d, F64), color_loss_vjp(*a, d, F32)
    W, den = w["base"] + w["color"] + w["pixel"], float(r64[3])
    out["d_cb"] = _k_spec(g64[0], g32[0], c["keep_cb"], (abs(d[0]) * w["base"] / W + abs(d[1])) / den, "k_l1")
    out["d_c"] = _k_spec(g64[1], g32[1], c["keep_c"], (abs(d[0]) * w["color"] / W + abs(d[2])) / den, "k_l1")
    return out


def sign_pattern(pred, gt):
    """sign(pred - gt) per element, flattened: -1 / 0 / 1 (the float64 difference of fp32 numbers is exact in sign)"""
    return torch.sign(pred.double() - gt.double()).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ #
# the step's loss assembly (exp_runner_blending.py:330-371 with the two L1 terms and the three regularisers)
# ------------------------------------------------------------------------------------------------------------------ #
SUMS5 = [[3.7, 120.0, 0.91, 77.0, 41.5], [0.0, 0.0, 0.0, 0.0, 0.0], [1e-3, 1.0, 5.0, 512.0, 500.0]]
NBLK = [1, 17, 1024, 1025]
N_RAYS = 512.0
D_TOTAL = 0.83
D_EXTRA = [0.0, 0.45, -0.6, 0.3, -0.21, 0.77, -1.9, 0.9]      # slot 0 is the total's own (d_total), slot 7 a constant output


def sums_errors(s, n_rays):
    """udf_renderer_blending.py:531-536, 553: the masked means of the composite sums"""
    return s[0] / (s[1] + 1e-5), s[2] / (s[3] + 1e-5), s[4] / n_rays


def step_loss(cb, c, gt, mask, sums5, n_rays, w, dtype):
    """-> out[8] = (total, cl, Lb, Lc, ge, gens, sparse, 0) as a tuple of 0-dim tensors, den.  sums5: [5], or the deferred
    form [nblk, 5] whose column sums are the five"""
    s = sums5.to(dtype)
    if s.dim() == 2:
        s = s.sum(0)
    cl, Lb, Lc, den = color_loss(cb, c, gt, mask, w, dtype)
    ge, gens, sp = sums_errors(s, n_rays)
    total = cl + gens * w["igr_ns"] + sp * w["sparse"] + ge * w["igr"]
    return (total, cl, Lb, Lc, ge, gens, sp, torch.zeros((), dtype=dtype)), den


def step_loss_vjp(cb, c, gt, mask, sums5, n_rays, w, d_total, d_extra, dtype):
    """d_total: a float or None (= 1); d_extra: 8 floats or None -> d_cb, d_c, d_sums [5]"""
    a, b = cb.to(dtype).clone().requires_grad_(True), c.to(dtype).clone().requires_grad_(True)
    s = sums5.to(dtype).clone().requires_grad_(True)
    out, _ = step_loss(a, b, gt, mask, s, n_rays, w, dtype)
    f = out[0] * (1.0 if d_total is None else d_total)
    if d_extra is not None:
        f = f + sum(out[k] * d_extra[k] for k in range(1, 8))
    f.backward()
    return a.grad, b.grad, s.grad


@functools.lru_cache(maxsize=None)
def sums_case(si, nblk=0):
    """SUMS5[si] as five sums (nblk = 0), or as [nblk, 5] non-negative partials whose fp32 column sums are close to them"""
    if nblk == 0:
        return torch.tensor(SUMS5[si])
    g = torch.Generator().manual_seed(100 * si + nblk)
    share = torch.rand(nblk, 5, generator=g) + 0.05
    return (share / share.sum(0, keepdim=True) * torch.tensor(SUMS5[si])[None, :]).float().contiguous()


def _d_sums_mag(s64, n_rays, w, d_total, d_extra):
    """|d_sums| with every term taken at its magnitude (d_total w and d_extra may cancel): what the roundings scale with"""
    g = abs(1.0 if d_total is None else d_total)
    dx = [0.0] * 8 if d_extra is None else [abs(x) for x in d_extra]
    dge, dgens, dsp = g * w["igr"] + dx[4], g * w["igr_ns"] + dx[5], g * w["sparse"] + dx[6]
    a, b = float(s64[1]) + 1e-5, float(s64[3]) + 1e-5
    return [dge / a, dge * abs(float(s64[0])) / (a * a), dgens / b, dgens * abs(float(s64[2])) / (b * b), dsp / n_rays]


@functools.lru_cache(maxsize=None)
def step_rows(N, mkind, wname, si, nblk=0, upstream="total"):
    """-> {output: spec} of step_loss_fwd (out0..out7, den, sums0..4 when deferred) and step_loss_bwd.  upstream: "total"
    (d_total alone), "null" (d_total NULL = 1, d_extra NULL), "extra" (both), "extra_null" (d_total NULL with d_extra)"""
    c, mask, w = color_case(N), mask_case(N, mkind), WEIGHTS[wname]
    sums = sums_case(si, nblk)
    a = (c["cb"], c["c"], c["gt"], mask, sums, N_RAYS, w)
    (o64, den64), (o32, den32) = step_loss(*a, F64), step_loss(*a, F32)
    g = torch.Generator().manual_seed(N + nblk)
    extra = []
    for _ in range(N_PERM):
        pc = _permute_elements((c["cb"], c["c"], c["gt"]), torch.randperm(3 * N, generator=g))
        pm = None if mask is None else mask[torch.randperm(N, generator=g)]
        ps = sums if nblk == 0 else sums[torch.randperm(nblk, generator=g)]
        extra.append(step_loss(*pc, pm, ps, N_RAYS, w, F32) + ((ps.sum(0) if nblk else ps),))
    out = {}
    for i, fl in enumerate(("total", "cl", "L", "L", "reg", "reg", "reg", "exact")):
        out["out%d" % i] = spec(o64[i], o32[i], [e[0][i] for e in extra], 1, rfloor(fl, o64[i]))
    out["den"] = spec(den64, den32, [e[1] for e in extra], 1, rfloor("den", den64))
    s64 = sums.double().sum(0) if nblk else sums.double()
    if nblk:
        s32 = sums.sum(0)
        for k in range(5):
            out["sums%d" % k] = spec(s64[k], s32[k], [e[2][k] for e in extra], 1, rfloor("sum", s64[k]))
    d_total = None if upstream in ("null", "extra_null") else D_TOTAL
    d_extra = D_EXTRA if upstream in ("extra", "extra_null") else None
    # the backward reads the five sums (not the partials): the fp32 sums the forward wrote stand in as exact inputs
    sb = sums if nblk == 0 else sums.double().sum(0).float()
    b = (c["cb"], c["c"], c["gt"], mask, sb, N_RAYS, w, d_total, d_extra)
    g64, g32 = step_loss_vjp(*b, F64), step_loss_vjp(*b, F32)
    gt_, dx = abs(1.0 if d_total is None else d_total), ([0.0] * 8 if d_extra is None else [abs(x) for x in d_extra])
    W, den = w["base"] + w["color"] + w["pixel"], float(den64)
    out["d_cb"] = _k_spec(g64[0], g32[0], c["keep_cb"], ((gt_ + dx[1]) * w["base"] / W + dx[2]) / den, "k_l1")
    out["d_c"] = _k_spec(g64[1], g32[1], c["keep_c"], ((gt_ + dx[1]) * w["color"] / W + dx[3]) / den, "k_l1")
    mags = _d_sums_mag(sb.double(), N_RAYS, w, d_total, d_extra)
    for k in range(5):
        out["d_sums%d" % k] = spec(g64[2][k], g32[2][k], (), 1, rfloor("d_sums", mags[k]))
    out["_sums_bwd"] = sb
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# the blending step's loss (loss/loss.py:105-133, :56-84; exp_runner_blending.py:313-315, 330-371)
# ------------------------------------------------------------------------------------------------------------------ #
RATIO = 0.3
BLEND_RAYS = [1, 10, 65, 341, 342, 1025]            # 3 N either side of 1024; N past 1024 for the per-ray loops
BLEND_COUNTS = ["0", "1", "3", "4", "10", "0.6N", "N"]       # valid rays: k = 0 for 1 and 3, k = 1 for 4


def trim_count(ratio, count):
    """k as the reference forms it: int(ratio * mask.sum()), a Python float times an int64 tensor (torch: float32)"""
    return int(ratio * torch.tensor(count, dtype=torch.int64))


def blend_loss(cb, c, pix, gt, err, patch_mask, weight_sum, sums5, n_rays, w, ratio, dtype, shuffle=None):
    """-> dict(m [N] bool, err_masked [N], out: the twelve outputs, keep [N] bool per ray).  err may require grad.
    shuffle: a generator; the kept errors are averaged in another order"""
    T = lambda t: t.to(dtype)
    cb, c, pix, gt, err = T(cb), T(c), T(pix), T(gt), T(err)
    # exp_runner_blending.py:315: (render patch_mask.float()[:, None] * (weight_sum > 0.5).float()) > 0
    m = (T(patch_mask)[:, None] * (T(weight_sum)[:, None] > 0.5).to(dtype)) > 0.0
    # ColorPatchLoss.forward (loss/loss.py:79-84)
    em = err * m[:, 0].to(dtype)
    es, idx = torch.sort(em, descending=True)
    ms = torch.index_select(m, 0, idx).clone()
    k = int(ratio * ms.sum())
    ms[:k] = False
    sel = es[ms.squeeze(-1)]
    if shuffle is not None and len(sel) > 1:
        sel = sel[torch.randperm(len(sel), generator=shuffle)]
    Lpatch = sel.mean()
    Lb, Lc, Lpix = _l1(cb, gt, None), _l1(c, gt, None), _l1(pix, gt, m)
    cl = (Lb * w["base"] + Lc * w["color"] + Lpix * w["pixel"]) / (w["base"] + w["color"] + w["pixel"]) + Lpatch * w["patch"]
    s = sums5.to(dtype)
    if s.dim() == 2:
        s = s.sum(0)
    ge, gens, sp = sums_errors(s, n_rays)
    total = cl + gens * w["igr_ns"] + sp * w["sparse"] + ge * w["igr"]
    keep = torch.zeros(len(err), dtype=torch.bool)
    keep[idx[ms.squeeze(-1)]] = True
    den_pix = m.sum() + 1e-4
    out = (total, cl, Lb, Lc, Lpix, Lpatch, ge, gens, sp, den_pix.to(dtype), torch.tensor(float(k), dtype=dtype),
           torch.tensor(float(ms.sum()), dtype=dtype))
    return dict(m=m[:, 0], err_masked=em, out=out, keep=keep, k=k, kept=int(ms.sum()), idx=idx)


def blend_loss_vjp(cb, c, pix, gt, err, patch_mask, weight_sum, sums5, n_rays, w, ratio, d_total, dtype):
    """-> d_cb, d_c, d_pix [N,3], d_err [N], d_sums [5] of out[0] d_total (None = 1)"""
    L = lambda t: t.to(dtype).clone().requires_grad_(True)
    a, b, p, e, s = L(cb), L(c), L(pix), L(err), L(sums5)
    r = blend_loss(a, b, p, gt, e, patch_mask, weight_sum, s, n_rays, w, ratio, dtype)
    (r["out"][0] * (1.0 if d_total is None else d_total)).backward()
    return a.grad, b.grad, p.grad, e.grad, s.grad


@functools.lru_cache(maxsize=None)
def blend_case(N, count):
    """the blending step's inputs with `count` valid rays: patch_mask in {0, 1} and weight_sum on both sides of 0.5 (a ray is
    valid when both say so; both ways of being invalid occur), err strictly positive and distinct on the valid rays.
    Asserts that the trim boundary is untied."""
    n_valid = dict(zip(BLEND_COUNTS, (0, 1, 3, 4, 10, int(round(0.6 * N)), N)))[count]
    assert n_valid <= N
    g = torch.Generator().manual_seed(9000 + 13 * N + n_valid)
    c = dict(color_case(N, third=True))
    valid = torch.zeros(N, dtype=torch.bool)
    valid[torch.randperm(N, generator=g)[:n_valid]] = True
    how = torch.randint(0, 3, (N,), generator=g)                   # an invalid ray: no patch, a weight sum <= 0.5, or both
    patch_mask = (valid | (how == 1)).float()
    ws_hi = 0.5 + 0.01 + 0.5 * torch.rand(N, generator=g)
    ws_lo = 0.5 * torch.rand(N, generator=g)
    ws_lo[::5] = 0.5                                               # exactly 0.5 is not > 0.5
    weight_sum = torch.where(valid | (how == 0), ws_hi, ws_lo)
    err = (0.05 + torch.rand(N, generator=g)).float()
    # distinct on the valid rays: redraw any duplicate
    while len(torch.unique(err[valid])) < int(valid.sum()):
        err = (0.05 + torch.rand(N, generator=g)).float()
    m = (patch_mask * (weight_sum > 0.5).float()) > 0
    assert torch.equal(m, valid) and bool((err[valid] > 0).all())
    k = trim_count(RATIO, n_valid)
    es = torch.sort(err * m.float(), descending=True)[0]
    assert k == 0 or k >= N or float(es[k - 1]) != float(es[k]), "the trim boundary is tied"
    c.update(err=err, patch_mask=patch_mask, weight_sum=weight_sum, n_valid=n_valid, k=k)
    return c


@functools.lru_cache(maxsize=None)
def blend_rows(N, count, wname, si, nblk=0, d_total=D_TOTAL):
    """-> {output: spec} of blend_loss_prepare (m, err_masked), blend_loss_fwd (out0..11, sums when deferred) and _bwd"""
    c, w, sums = blend_case(N, count), WEIGHTS[wname], sums_case(si, nblk)
    a = (c["cb"], c["c"], c["pix"], c["gt"], c["err"], c["patch_mask"], c["weight_sum"], sums, N_RAYS, w, RATIO)
    r64, r32 = blend_loss(*a, F64), blend_loss(*a, F32)
    assert r64["k"] == r32["k"] == c["k"] and torch.equal(r64["keep"], r32["keep"])
    g = torch.Generator().manual_seed(N + nblk + 1)
    extra = []
    for _ in range(N_PERM):
        pc = _permute_elements((c["cb"], c["c"], c["pix"], c["gt"]), torch.randperm(3 * N, generator=g))
        ps = sums if nblk == 0 else sums[torch.randperm(nblk, generator=g)]
        e = blend_loss(*pc, *a[4:7], ps, N_RAYS, w, RATIO, F32, shuffle=g)
        extra.append((e["out"], (ps.sum(0) if nblk else ps)))
    out = dict(m=spec(r64["m"].double(), r32["m"].float(), (), 64, 0.0), err_masked=spec(r64["err_masked"], r32["err_masked"], (), 64, 0.0))
    names = ("blend_total", "blend_cl", "blend_L", "blend_L", "L", "Lpatch", "reg", "reg", "reg", "den", "exact", "exact")
    for i, fl in enumerate(names):
        fv = r64["out"][i]
        floor = rfloor(fl, fv) if bool(torch.isfinite(fv)) else 0.0
        out["out%d" % i] = spec(fv, r32["out"][i], [e[0][i] for e in extra], 1, floor)
    if nblk:
        s64, s32 = sums.double().sum(0), sums.sum(0)
        for k in range(5):
            out["sums%d" % k] = spec(s64[k], s32[k], [e[1][k] for e in extra], 1, rfloor("sum", s64[k]))
    sb = sums if nblk == 0 else sums.double().sum(0).float()
    b = a[:7] + (sb, N_RAYS, w, RATIO, d_total)
    g64, g32 = blend_loss_vjp(*b, F64), blend_loss_vjp(*b, F32)
    gt_ = abs(1.0 if d_total is None else d_total)
    W = w["base"] + w["color"] + w["pixel"]
    dens = (3.0 * N, 3.0 * N, float(r64["out"][9]))
    for i, (nm, wk) in enumerate((("cb", "base"), ("c", "color"), ("pix", "pixel"))):
        out["d_" + nm] = spec(g64[i].reshape(-1), g32[i].reshape(-1), (), 64 * 3, rfloor("blend_k", gt_ * w[wk] / W / dens[i]),
                              c["keep_" + nm], one_draw=True)
    kept = max(r64["kept"], 1)
    out["d_err"] = spec(g64[3], g32[3], (), 64, rfloor("d_err", gt_ * w["patch"] / kept), one_draw=True)
    mags = _d_sums_mag(sb.double(), N_RAYS, w, d_total, None)
    for k in range(5):
        out["d_sums%d" % k] = spec(g64[4][k], g32[4][k], (), 1, rfloor("d_sums", mags[k]))
    out["_ref"] = r64
    out["_nan"] = tuple("out%d" % i for i in range(12) if not bool(torch.isfinite(r64["out"][i])))
    out["_sums_bwd"] = sb
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# the matrix: every size with every mask; the other knobs cycle with strides that tests/test_loss_ref.py checks for cover
# ------------------------------------------------------------------------------------------------------------------ #
WNAMES = list(WEIGHTS)
UPSTREAMS = ["total", "null", "extra", "extra_null"]


def _cases():
    color, step = [], []
    for ni, N in enumerate(RAYS):
        for mi, mk in enumerate(MASKS):
            i = 5 * ni + mi
            # (N, mask, weights, upstream triple, weights by value or from the device vector)
            color.append((N, mk, WNAMES[i % 3], (i // 3) % 3, ("value", "dev")[(ni + mi) % 2]))
            # (N, mask, weights, sums vector, nblk of the deferred form or 0, upstream, value / dev)
            step.append((N, mk, WNAMES[i % 3], (i // 3) % 3, ([0] + NBLK)[(2 * i + i // 5) % 5], UPSTREAMS[(i + i // 4) % 4],
                         ("value", "dev")[(ni + mi) % 2]))
    blend = []
    for ci, count in enumerate(BLEND_COUNTS):
        for ni, N in enumerate(BLEND_RAYS):
            if dict(zip(BLEND_COUNTS, (0, 1, 3, 4, 10, 0, 0)))[count] > N:
                continue
            i = 6 * ci + ni
            # (N, count, weights, sums vector, nblk, d_total or None = NULL)
            blend.append((N, count, WNAMES[i % 3], (i // 3) % 3, ([0] + NBLK)[(2 * i + i // 5) % 5], (D_TOTAL, None)[(i + i // 6) % 2]))
    return color, step, blend


COLOR_CASES, STEP_CASES, BLEND_CASES = _cases()
SHARD_CASES = [(N, mk, WNAMES[(i + j) % 3]) for i, N in enumerate(RAYS[1:]) for j, mk in enumerate(("none", "random", "zeros"))]


@functools.lru_cache(maxsize=None)
def shard_rows(N, mkind, wname):
    """color_loss_sums of two shards (the first N // 3 rays and the rest), added, then color_loss_finish: against the float64
    loss of the whole batch"""
    full = color_rows(N, mkind, wname, 0)
    return {k: full[k] for k in ("total", "Lb", "Lc", "den")}
