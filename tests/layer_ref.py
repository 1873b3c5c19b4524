"""The per-layer path (the 13 epilogues of gemm_nn, the per-point kernels of csrc/rays_embed.hip around it, csrc/optim.hip)
as plain torch functions of a dtype, the generators of the inputs the layer matrix runs on, the margins of the discrete
decisions, and the tile-wise bound.  No GPU in here.

Every operation is restated from the oracle (oracle/udf_oracle.py), models/fields.py and torch itself -- never from the
kernels -- and evaluated twice on the same fp32-drawn inputs: in float64 (the reference) and in float32 (`e_ref`: how far a
correct fp32 evaluation sits from float64).  tests/test_layer_ref.py checks the restatements against autograd.

Bound, per tile (a 32 x 32 tile of a GEMM output, a 64-point block of a per-point kernel, a tensor of Adam), in the tile's
max norm:  err <= min(max(FACTOR e_ref, floor), CAP max|ref|).  floor is 0 in every tile of more than SMALL_TILE = 32 kept
elements: those are held to FACTOR e_ref alone.  A tile of one to 32 elements (row 128 of M = 130, the last row of out = 257,
one ray point, a one-element row) leaves e_ref the largest of a handful of draws, and the rows that have such tiles carry a
floor for them, derived from the row's own arithmetic (below).

Ties.  A discrete decision whose float64 quantity is within MARGIN of its threshold is left out of the comparison (the sign
of the UDF head's column 0, pred - gt against 0, the clamps of the scalars); at most TIE_CAP of a case's rows."""
import functools
import math

import torch
import torch.nn.functional as F

from composite_ref import CAP, FACTOR, MARGIN
from oracle import udf_oracle as O

F32, F64 = torch.float32, torch.float64
TIE_CAP = 0.10
WINDOW = (1e-4, 1e-2)            # the softplus window: 1e-4 <= exp(100 a) <= 1e-2
WINDOW_FACTOR = 4.0

# Floors (absolute, in the tile's max norm), each derived from the row's own arithmetic.  They count in tiles of at most
# SMALL_TILE kept elements only (`tiles`): the ragged tiles of the GEMM rows (gemm_floor), of the weight-norm rows (wn_floors) and
# of the ray points o + d t (ray_floor), and the one-element rows of the scalars and of sums_errors (scalar_floor,
# quotient_floor).  The one floor of another kind is the chain's softplus in the window (CHAIN_SOFTPLUS_FLOOR).
ULP1 = 2.0 ** -23


# The chain kernels' softplus is log(1 + exp2(-|t|)) / 100 from the hardware transcendentals, by design accurate in ABSOLUTE
# terms only: z <= 1 carries <= 2^-24 of its own and the sum 1 + z rounds by <= 2^-24, so log(1 + z) is off by
# <= 2^-23 and h by 2^-23 / 100, whatever the size of h.  In the window h itself is 1e-6 ... 1e-4 and e_ref ~ 6e-11.
CHAIN_SOFTPLUS_FLOOR = ULP1 / 100.0


def scalar_floor(value):
    """a row of ONE element, exp(10 p) times exact factors: the product 10 p (|10 p| <= 14) rounds by <= ulp(14) / 2 =
    4.8e-7, which the exponential turns into that much of the value, and expf adds <= 2 ulp = 2.4e-7.  e_ref is a single
    draw of the same roundings and can be exact by luck."""
    return 7.2e-7 * abs(float(value))


def quotient_floor(value):
    """a row of ONE element formed by a sum, a product and a quotient (sums_errors): <= 4 roundings of 2^-24 each"""
    return 4.0 * 2.0 ** -24 * abs(float(value))


# ------------------------------------------------------------------------------------------------------------------ #
# softplus(beta = 100, threshold = 20) and its derivatives from the pre-activation
# ------------------------------------------------------------------------------------------------------------------ #
def sp(a):
    return O.softplus100(a)


def sp_s(a):
    """softplus' as autograd forms it: 1 above the threshold, sigmoid(100 a) below"""
    t = 100.0 * a
    return torch.where(t > 20.0, torch.ones_like(a), torch.sigmoid(t))


def sp_om(a):
    """1 - softplus', without the cancellation"""
    t = 100.0 * a
    return torch.where(t > 20.0, torch.zeros_like(a), torch.sigmoid(-t))


def sp_d2(a):
    """softplus'' = 100 s (1 - s)"""
    return 100.0 * sp_s(a) * sp_om(a)


def stored(apre, xscale):
    """the activation a forward sweep stores: softplus(a) / xscale, formed in float64 and rounded once to fp32"""
    return (sp(apre.double()) / xscale).float()


def window_points(n=200001):
    """fp32 pre-activations covering the window evenly in log z"""
    return torch.linspace(math.log(WINDOW[0]) / 100.0, math.log(WINDOW[1]) / 100.0, n, dtype=F64).float()


def relmax(a, b):
    """worst element-relative error of a against b (float64)"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b).abs() / b.abs()).max())


@functools.lru_cache(maxsize=None)
def window_figures():
    """what torch's own fp32 evaluation loses over the window, element-relative: `softplus` (F.softplus in fp32) and
    `s_from_h` (softplus' recovered from the exactly rounded stored activation as -expm1(-100 xscale h), worst of
    xscale 1 and sqrt 2); pinned by tests/test_layer_ref.py, and WINDOW_FACTOR times them is the GPU's window bar"""
    a = window_points()
    out = dict(softplus=relmax(sp(a), sp(a.double())), s_from_pre=relmax(sp_s(a), sp_s(a.double())))
    worst = 0.0
    for xs in (1.0, 1.4142135):
        x = (torch.tensor(100.0) * torch.tensor(xs)) * stored(a, xs)
        worst = max(worst, relmax(-torch.expm1(-x), sp_s(a.double())))
    out["s_from_h"] = worst
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# the 13 epilogues of epilogue_store, as functions of v = A @ B (+ bias)
# ------------------------------------------------------------------------------------------------------------------ #
EPILOGUES = ["NONE", "SOFTPLUS", "RELU", "MUL", "MULMASK", "TANGENT", "BWD", "SIGMOID", "UDFHEAD", "SKIPSPLIT", "RELU_DUAL",
             "ADDMASK", "MULSP"]
HEADS = {0: "abs", 1: "square", 2: "sdf"}


def udf_head(v0, kind):
    """udf_out of fields.py:184-190 and its derivative"""
    if kind == "abs":
        return v0.abs(), torch.sign(v0)
    if kind == "square":
        return v0 * v0, 2.0 * v0
    return v0, torch.ones_like(v0)


def epilogue(epi, v, o, dtype):
    """-> {"C1": ..., "C2": ..., "C3": ...} (the outputs the launch writes) in `dtype`.  o: scale, xscale, iparam, apre (the
    pre-activation behind the stored activation X1), X1 (multiplier / mask), X2, c2 / c3 / x2 (which optional arrays the
    launch is given)."""
    T = lambda k: o[k].to(dtype)
    sc, ip = o.get("scale", 1.0), o.get("iparam", 0)
    if epi == "NONE":
        return dict(C1=v * sc)
    if epi == "SOFTPLUS":
        out = dict(C1=sp(v) * sc)
        if o.get("c2"):
            out["C2"] = sp_s(v)
        return out
    if epi == "RELU":
        return dict(C1=torch.relu(v) * sc)
    if epi == "MUL":
        return dict(C1=v * T("X1") * sc)
    if epi == "MULMASK":
        return dict(C1=torch.where(o["X1"] > 0, v * sc, torch.zeros_like(v)))
    if epi == "MULSP":
        return dict(C1=v * sp_s(T("apre")) * sc)
    if epi == "TANGENT":
        a = T("apre")
        return dict(C1=v * sp_s(a) * sc, C2=v * T("X2") * 100.0 * sp_om(a))
    if epi == "BWD":
        c = v * sc * sp_s(T("apre"))
        return dict(C1=c + T("X2") if o.get("x2") else c)
    if epi == "SIGMOID":
        sig = torch.sigmoid(v[:, :ip])
        out = dict(C1=sig if o.get("c3") else torch.cat([sig, v[:, ip:]], 1))
        if o.get("c2"):
            out["C2"] = sig
        if o.get("c3"):
            out["C3"] = v[:, ip:]
        return out
    if epi == "UDFHEAD":
        hv, hm = udf_head(v[:, 0], HEADS[ip])
        out = dict(C2=(hv * sc)[:, None], C3=hm[:, None])
        if v.shape[1] > 1:
            out["C1"] = v[:, 1:]
        return out
    if epi == "SKIPSPLIT":
        return dict(C1=v[:, :ip] * sp_s(T("apre")[:, :ip]) * sc, C2=v[:, ip:] * sc)
    if epi == "RELU_DUAL":
        h = torch.relu(v)
        return dict(C1=h, C2=h) if o.get("c2") else dict(C1=h)
    if epi == "ADDMASK":
        return dict(C1=torch.where(o["X1"] > 0, (v + T("X2")) * sc, torch.zeros_like(v)))
    raise KeyError(epi)


# (M, N, K): every epilogue sees M and N on both sides of 32 and 64 and three K; (256, 65): 8 block tiles with a ragged N
# (xcd_swizzle permutes); (512, 130): 24 tiles, tiles_n = 3
SHAPES = [(1, 1, 32), (33, 13, 64), (64, 33, 288), (65, 64, 32), (130, 65, 64), (256, 65, 32), (512, 130, 64)]
SIGMOID_SHAPES = [(33, 3, 32), (64, 6, 64), (130, 35, 288)]


def _v(name, epi, shapes=None, **o):
    return dict(name=name, epi=epi, shapes=shapes or SHAPES, o=o)


VARIANTS = [
    _v("NONE", "NONE", scale=0.7),
    _v("SOFTPLUS_c2", "SOFTPLUS", scale=0.5, c2=True),
    _v("SOFTPLUS", "SOFTPLUS", scale=1.0, c2=False),
    _v("RELU", "RELU", scale=0.7),
    _v("MUL", "MUL", scale=0.7),
    _v("MULMASK", "MULMASK", scale=0.7),
    _v("MULSP", "MULSP", scale=0.7, xscale=1.4142135),
    _v("TANGENT", "TANGENT", scale=0.7, xscale=1.4142135),
    _v("BWD_x2", "BWD", scale=0.7, xscale=1.4142135, x2=True),
    _v("BWD", "BWD", scale=0.7, xscale=1.0, x2=False),
    _v("UDFHEAD_abs", "UDFHEAD", scale=1.3, iparam=0),
    _v("UDFHEAD_square", "UDFHEAD", scale=1.3, iparam=1),
    _v("UDFHEAD_sdf", "UDFHEAD", scale=1.3, iparam=2),
    _v("SKIPSPLIT_25", "SKIPSPLIT", scale=0.7, xscale=1.4142135, iparam=25),
    _v("SKIPSPLIT_64", "SKIPSPLIT", scale=0.7, xscale=1.4142135, iparam=64),
    _v("RELU_DUAL_c2", "RELU_DUAL", c2=True),
    _v("RELU_DUAL", "RELU_DUAL", c2=False),
    _v("ADDMASK", "ADDMASK", scale=0.7),
    _v("SIGMOID_c2_c3", "SIGMOID", SIGMOID_SHAPES + SHAPES, iparam=3, c2=True, c3=True),
    _v("SIGMOID_c3", "SIGMOID", SIGMOID_SHAPES, iparam=3, c2=False, c3=True),
    _v("SIGMOID_c2", "SIGMOID", SIGMOID_SHAPES, iparam=3, c2=True, c3=False),
    _v("SIGMOID", "SIGMOID", SIGMOID_SHAPES + SHAPES[3:5], iparam=3, c2=False, c3=False),
]
VARIANT = {v["name"]: v for v in VARIANTS}
S_FROM_H = ("MULSP", "TANGENT", "BWD", "SKIPSPLIT")
K_PERMS = 3


def gemm_floor(epi, v64, mag, o, r64):
    """The floor of a GEMM row, element-wise.  v is an fp32 sum of K products: whatever the order, it is not known below
    one ulp of the magnitude it was summed at, mag = sum_k |a_k b_k| + |bias|; the epilogue passes that on with its own
    gain and rounds its result once more.  So an element may be off by |f(v + 2^-23 mag) - f(v)| + 2^-23 |f(v)|, and the
    floor is GEMM_FLOOR_ULPS times that.  It counts only in the ragged tiles of a few elements (row 128 of M = 130, column 64
    of N = 65), where the largest of so few draws of e_ref can sit far under an ulp; a tile of more than SMALL_TILE elements is held to
    4 e_ref alone (`tiles`)."""
    moved = epilogue(epi, v64 + ULP1 * mag, o, F64)
    return {k: GEMM_FLOOR_ULPS * ((moved[k] - r).abs() + ULP1 * r.abs()) for k, r in r64.items()}


GEMM_FLOOR_ULPS = 2.0


@functools.lru_cache(maxsize=None)
def gemm_case(name, si):
    """inputs (fp32), reference (float64), fp32 evaluation and the rows kept of shape `si` of VARIANT[name]; shared"""
    var = VARIANT[name]
    epi, (M, N, K) = var["epi"], var["shapes"][si]
    g = torch.Generator().manual_seed(1000 * EPILOGUES.index(epi) + 17 * si + len(name))
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g) * 0.1
    bias = torch.randn(N, generator=g)
    if epi == "SOFTPLUS":
        # pre-activations of sigma 0.13 (6 sigma < 0.8): both sides of the threshold 100 v = 20 are reached, and softplus(v)
        # stays inside fp32's normal range -- below v = -0.87 no fp32 evaluation, torch's included, stores anything but 0
        B, bias = B / math.sqrt(K), bias * 0.08
    o = dict(var["o"])
    if epi in S_FROM_H:
        # softplus' from the stored activation: pre-activations over all three branches (100 h < 0.01, middle, > 20)
        o["apre"] = torch.randn(M, N, generator=g) * 0.15
    if epi in ("MUL", "MULMASK", "ADDMASK"):
        x1 = torch.randn(M, N, generator=g)
        x1[torch.rand(M, N, generator=g) < 0.2] = 0.0          # exact zeros, negatives and positives
        o["X1"] = x1
    if epi in ("TANGENT", "ADDMASK") or o.get("x2"):
        o["X2"] = torch.randn(M, N, generator=g)
    use_bias = epi not in ("TANGENT", "BWD")                    # the reverse sweeps carry none
    v64 = A.double() @ B.double() + (bias.double() if use_bias else 0.0)
    v32 = A @ B + (bias if use_bias else 0.0)
    keep = torch.ones(M, dtype=torch.bool)
    if epi == "UDFHEAD" and o["iparam"] == 0:
        keep = v64[:, 0].abs() > MARGIN                          # the sign of column 0
    # the K sum is a reduction whose order is not torch's: further fp32 evaluations with the k order permuted
    extra = []
    for _ in range(K_PERMS):
        pk = torch.randperm(K, generator=g)
        extra.append(epilogue(epi, A[:, pk] @ B[pk, :] + (bias if use_bias else 0.0), o, F32))
    r64 = epilogue(epi, v64, o, F64)
    mag = A.double().abs() @ B.double().abs() + (bias.double().abs() if use_bias else 0.0)
    return dict(M=M, N=N, K=K, epi=epi, A=A, B=B, bias=bias if use_bias else None, o=o, v64=v64, v32=v32, keep=keep,
                r64=r64, r32=epilogue(epi, v32, o, F32), r32_extra=extra, floor=gemm_floor(epi, v64, mag, o, r64))


@functools.lru_cache(maxsize=None)
def window_case(epi):
    """a 64 x 32 launch whose product is exact (B = the identity), so that the element-relative error is the epilogue's
    alone.  SOFTPLUS: the pre-activations v = A lie in the window.  The s-from-h epilogues: v = A is any fp32 number and
    the stored activations come from pre-activations in the window."""
    g = torch.Generator().manual_seed(77 + EPILOGUES.index(epi))
    M, N, K = 64, 32, 32
    lo, hi = math.log(WINDOW[0] * 1.001) / 100.0, math.log(WINDOW[1] * 0.999) / 100.0
    win = (lo + (hi - lo) * torch.rand(M, N, generator=g, dtype=F64)).float()
    o = dict(scale=0.7, xscale=1.4142135)
    if epi == "SOFTPLUS":
        A, o = win, dict(scale=1.0, c2=True)
    else:
        A = torch.randn(M, K, generator=g) + 2.0 * torch.sign(torch.randn(M, K, generator=g))     # away from 0
        o["apre"] = win
        if epi == "TANGENT":
            o["X2"] = torch.randn(M, N, generator=g)
        if epi == "SKIPSPLIT":
            o["iparam"] = 25
    B = torch.eye(K)
    z = torch.exp(100.0 * win.double())
    assert float(z.min()) >= WINDOW[0] and float(z.max()) <= WINDOW[1]
    v64 = A.double()
    return dict(M=M, N=N, K=K, epi=epi, A=A, B=B, bias=None, o=o, v64=v64, r64=epilogue(epi, v64, o, F64),
                r32=epilogue(epi, A.clone(), o, F32), r32_extra=[], keep=torch.ones(M, dtype=torch.bool),
                floor={k: 0.0 for k in ("C1", "C2", "C3")})      # exact products: no floor


def branch_shares(apre, xscale):
    """share of stored activations in each branch of the s-from-h recovery: x = 100 xscale h < 0.01, middle, > 20"""
    x = 100.0 * xscale * stored(apre, xscale).double()
    return float((x < 0.01).float().mean()), float(((x >= 0.01) & (x <= 20)).float().mean()), float((x > 20).float().mean())


# ------------------------------------------------------------------------------------------------------------------ #
# sampling (udf_renderer_blending.py:605-630, 164-173, 352-357)
# ------------------------------------------------------------------------------------------------------------------ #
def coarse_z(near, far, S, t_rand, center, dtype):
    """near / far [N,1] or [1,1], t_rand [N,1] or None -> z [N or 1 -> N, S], sample_dist (0-dim)"""
    near, far = near.to(dtype), far.to(dtype)
    z = near + (far - near) * torch.linspace(0.0, 1.0, S, dtype=dtype)[None, :]
    if t_rand is not None:
        t = t_rand.to(dtype)
        if center:
            t = t - 0.5
        z = z + t * 2.0 / S
    return z, ((far - near) / S).mean()


def sample_dist_permuted(near, far, S, perm):
    """the fp32 mean with its operands in another order"""
    return ((far[perm] - near[perm]) / S).mean()


def outside_z(far, lin, n_samples, dtype):
    """far [N,1], lin [n_out] -> far / flip(lin) + 1 / n_samples"""
    return far.to(dtype) / torch.flip(lin.to(dtype), dims=[-1]) + 1.0 / n_samples


def ray_points(o, d, z, sample_dist, mode, dtype):
    """mode 0: o + d z; 1: interval mid points (last interval = sample_dist); 2: + the inverted sphere (x / r, 1 / r)"""
    o, d, z = o.to(dtype), d.to(dtype), z.to(dtype)
    if mode >= 1:
        dists = torch.cat([z[:, 1:] - z[:, :-1], sample_dist.to(dtype).reshape(1, 1).expand(z.shape[0], 1)], -1)
        z = z + dists * 0.5
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    if mode == 2:
        r = torch.linalg.norm(pts, ord=2, dim=-1, keepdim=True).clip(1.0, 1e10)
        pts = torch.cat([pts / r, 1.0 / r], -1)
    return pts.reshape(-1, pts.shape[-1])


def ray_floor(o, pts64):
    """o + d t is one product and one sum, which the device contracts into one fma and the host rounds twice: either way
    an ulp of the larger of |o| and |d t| at most.  A block of one point (3 numbers) leaves e_ref the largest of three
    draws, so the row has this floor: 2^-23 (|o| + |d t|), element-wise (modes 0 and 1)."""
    o = o.double()
    S = pts64.shape[0] // o.shape[0]
    oo = o[:, None, :].expand(o.shape[0], S, 3).reshape(-1, 3)
    return ULP1 * (oo.abs() + (pts64 - oo).abs())


# ------------------------------------------------------------------------------------------------------------------ #
# encoding
# ------------------------------------------------------------------------------------------------------------------ #
def _rows(x, xdiv, P):
    return x.repeat_interleave(xdiv, 0)[:P]


def posenc(x, L, in_scale, xdiv, P, scale, dtype):
    return O.posenc(_rows(x.to(dtype), xdiv, P) * in_scale, L) * scale


def posenc_jvp(x, v, L, in_scale, xdiv, P, scale, dtype):
    xr = _rows(x.to(dtype), xdiv, P)
    return torch.autograd.functional.jvp(lambda t: O.posenc(t * in_scale, L), xr, v.to(dtype))[1] * scale


def posenc_vjp(x, L, in_scale, s1, c1, s2, c2, dtype):
    de = s1.to(dtype) * c1
    if s2 is not None:
        de = de + s2.to(dtype) * c2
    return torch.autograd.functional.vjp(lambda t: O.posenc(t * in_scale, L), x.to(dtype), de)[1]


def copy_cols(src, sdiv, ncols, P, scale, dtype):
    return _rows(src.to(dtype), sdiv, P)[:, :ncols] * scale


# ------------------------------------------------------------------------------------------------------------------ #
# head kernels
# ------------------------------------------------------------------------------------------------------------------ #
def udf_grad_seed(sign, wrow, apre, inv_scale, dtype):
    """d udf / d a of the last hidden layer: sign[p] W_last[0, c] inv_scale softplus'(a[p, c])  (fields.py:219-231)"""
    return sign.to(dtype)[:, None] * wrow.to(dtype)[None, :] * inv_scale * sp_s(apre.to(dtype))


def udf_head_bwd(sign, dudf, dfeat, scale, P, Fw, dtype):
    c0 = sign.to(dtype) * scale * dudf.to(dtype) if dudf is not None else torch.zeros(P, dtype=dtype)
    rest = dfeat.to(dtype) if dfeat is not None else torch.zeros(P, Fw, dtype=dtype)
    return torch.cat([c0[:, None], rest], 1)


def signed_colsum(sign, R, scale, out0, dtype, perm=None):
    s, r = sign.to(dtype), R.to(dtype)
    if perm is not None:
        s, r = s[perm], r[perm]
    return out0.to(dtype) + (s[:, None] * r).sum(0) * scale


def sigmoid_head_bwd(y, dy, dy_extra, draw, nraw, ldo, dtype):
    """[(dy + dy_extra) y (1 - y), draw, zeros up to ldo]"""
    y = y.to(dtype)
    d = torch.zeros_like(y)
    if dy is not None:
        d = d + dy.to(dtype)
    if dy_extra is not None:
        d = d + dy_extra.to(dtype)
    raw = draw.to(dtype) if draw is not None else torch.zeros(y.shape[0], nraw, dtype=dtype)
    return torch.cat([d * y * (1.0 - y), raw, torch.zeros(y.shape[0], ldo - y.shape[1] - nraw, dtype=dtype)], 1)


POINTS = [1, 63, 64, 65, 255, 257, 999]


@functools.lru_cache(maxsize=None)
def seed_case(P, C):
    """udf_grad_seed inputs: pre-activations over all three branches of the recovery (x < 0.01, the middle, x > 20)"""
    g = torch.Generator().manual_seed(31 * P + C)
    sign = torch.sign(torch.randn(P, generator=g))
    return dict(sign=sign, wrow=torch.randn(C, generator=g), apre=torch.randn(P, C, generator=g) * 0.15)


@functools.lru_cache(maxsize=None)
def l1_case(n):
    """pred, gt [n, 3] with every seventh element equal; keep: elements whose sign(pred - gt) is no tie"""
    g = torch.Generator().manual_seed(97 + n)
    pred, gt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    gt.reshape(-1)[::7] = pred.reshape(-1)[::7]
    d = (pred.double() - gt.double()).reshape(-1)
    return dict(pred=pred, gt=gt, d_out=torch.tensor([0.37]), keep=(d == 0) | (d.abs() > MARGIN))


# ------------------------------------------------------------------------------------------------------------------ #
# weight norm (torch.nn.utils.weight_norm, dim 0) with the packed column order
# ------------------------------------------------------------------------------------------------------------------ #
def wn_pack(v, g, perm, dtype):
    """-> W [out, in] in packed column order (W[:, perm[i]] = weight[:, i]), 1 / |v|_row (None for a plain Linear)"""
    v = v.to(dtype)
    if g is None:
        W, inv = v, None
    else:
        W = torch._weight_norm(v, g.to(dtype).reshape(-1, 1), 0)
        inv = 1.0 / torch.linalg.norm(v, dim=1)
    if perm is not None:
        Wp = torch.zeros_like(W)
        Wp[:, perm.long()] = W
        W = Wp
    return W, inv


def wn_unpack(dWp, v, g, perm, dtype):
    """packed dW [out, in] -> (dv, dg) by autograd through weight_norm"""
    dW = dWp.to(dtype)
    if perm is not None:
        dW = dW[:, perm.long()]
    if g is None:
        return dW, None
    vv = v.to(dtype).clone().requires_grad_(True)
    gg = g.to(dtype).reshape(-1, 1).clone().requires_grad_(True)
    (torch._weight_norm(vv, gg, 0) * dW).sum().backward()
    return vv.grad, gg.grad.reshape(-1)


def wn_floors(L, use_g, perm):
    """element-wise floors of the weight-norm rows.  A row of one or a few elements (out = 1, the last row of out = 33 /
    257) leaves e_ref the largest of a handful of draws.  W = v g / |v|: the sum of squares, the root, the reciprocal, g inv
    and the product round once each -- 5 half-ulps, 3 ulp of the element.  dg = <dW, v> inv and dv = g inv dW - v g inv^3
    <dW, v> hold a dot product, not known below an ulp of sum |dW v|: 2 ulp of that, through the same factors."""
    v, dW = L["v"].double(), L["dW"].double()
    if not use_g:
        z = torch.zeros_like(v)
        return dict(W=z, Wt=z.t(), inv_norm=None, dv=z, dg=None)
    g = L["g"].double()
    inv = 1.0 / torch.linalg.norm(v, dim=1)
    W = wn_pack(L["v"], L["g"], perm, F64)[0]
    dot = (dW * v).abs().sum(1)
    return dict(W=3 * ULP1 * W.abs(), Wt=3 * ULP1 * W.abs().t(), inv_norm=2 * ULP1 * inv, dg=2 * ULP1 * dot * inv,
                dv=2 * ULP1 * ((g * inv)[:, None] * dW.abs() + v.abs() * (g * inv ** 3 * dot)[:, None]))


WN_OUT, WN_IN = [1, 31, 33, 257], [3, 39, 65, 257]
# the multi-layer tables: (out, in, weight_norm, permuted); outs are no multiples of 32 or 4
WN_TABLE = [(33, 39, True, True), (1, 65, True, False), (257, 3, False, True), (31, 257, True, False), (70, 65, False, False)]


@functools.lru_cache(maxsize=None)
def wn_layer(out, inp, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(v=torch.randn(out, inp, generator=g), g=torch.rand(out, generator=g) + 0.5,
                perm=torch.randperm(inp, generator=g).int(), dW=torch.randn(out, inp, generator=g),
                db=torch.randn(out, generator=g))


# ------------------------------------------------------------------------------------------------------------------ #
# scalars and small losses
# ------------------------------------------------------------------------------------------------------------------ #
BETA_HI = 1.0 / 0.00005


def scalars(var, beta, gamma, beta_hi, d_scal, dtype):
    """-> scal [3] (inv_s, beta, gamma: the oracle's, clipped as at the call sites), recip [2], d_param [3] by autograd"""
    p = [t.to(dtype).clone().requires_grad_(True) for t in (var, beta, gamma)]
    scal = torch.cat([O.inv_s_of({"variance": p[0]}).reshape(1), O.beta_of({"beta": p[1]}, 1.0 / beta_hi).reshape(1),
                      O.gamma_of({"gamma": p[2]}).reshape(1)])
    (scal * d_scal.to(dtype)).sum().backward()
    return scal.detach(), 1.0 / scal.detach()[:2], torch.cat([q.grad.reshape(1) for q in p])


def scalar_ties(var, beta, gamma, beta_hi):
    """[3] bool: exp(10 p) within MARGIN (relative) of a clamp -- the derivative's decision"""
    out = []
    for q, cl in ((var, (1e-6, 1e6)), (beta, (1e-6, 1e6, beta_hi)), (gamma, (1e-6, 1e6))):
        e = float(torch.exp(10.0 * q.double()))
        out.append(any(abs(e / c - 1.0) < MARGIN for c in cl))
    return torch.tensor(out)


def _at(c, rel):
    """the fp32 parameter whose exp(10 p) is c (1 + rel)"""
    return torch.tensor([math.log(c * (1.0 + rel)) / 10.0], dtype=F64).float()


# (variance, beta, gamma) triples: at, just inside and just outside each clamp (1e-6, 1e6; beta_hi for beta)
SCALAR_CASES = [(_at(a, r), _at(b, r2), _at(c, r3)) for (a, r), (b, r2), (c, r3) in [
    ((0.3, 0), (40.0, 0), (20.0, 0)),
    ((1e-6, 0), (1e-6, 0), (1e-6, 0)), ((1e-6, 1e-3), (1e-6, 1e-3), (1e-6, 1e-3)), ((1e-6, -1e-3), (1e-6, -1e-3), (1e-6, -1e-3)),
    ((1e6, 0), (BETA_HI, 0), (1e6, 0)), ((1e6, 1e-3), (BETA_HI, 1e-3), (1e6, 1e-3)), ((1e6, -1e-3), (BETA_HI, -1e-3), (1e6, -1e-3)),
]]
SCALAR_TIES = 7                       # derivatives whose parameter sits AT a clamp (3 + 3 + 1 of the 30): left out, values kept
SCALAR_CASES_HI = [(_at(0.3, 0), _at(1e6, r), _at(20.0, 0)) for r in (0, 1e-3, -1e-3)]     # run with beta_hi = 2e6


def l1_sum(pred, gt, d_out, dtype, perm=None):
    p = pred.to(dtype).reshape(-1)
    q = gt.to(dtype).reshape(-1)
    if perm is not None:
        p, q = p[perm], q[perm]
    p = p.clone().requires_grad_(True)
    s = F.l1_loss(p, q, reduction="sum")
    (s * d_out.to(dtype)).sum().backward()
    return s.detach(), p.grad


def sums_errors(sums, n_rays, d_err, dtype):
    """masked means of the loss: sums[0] / (sums[1] + 1e-5), sums[2] / (sums[3] + 1e-5), sums[4] / n_rays, and the VJP"""
    s = sums.to(dtype).clone().requires_grad_(True)
    err = torch.stack([s[0] / (s[1] + 1e-5), s[2] / (s[3] + 1e-5), s[4] / n_rays])
    (err * d_err.to(dtype)).sum().backward()
    return err.detach(), s.grad


# ------------------------------------------------------------------------------------------------------------------ #
# Adam (torch.optim.Adam, single-tensor, no amsgrad / weight decay)
# ------------------------------------------------------------------------------------------------------------------ #
ADAM_SIZES = [1, 1023, 1024, 1025, 4097]
ADAM_STEPS, ADAM_LATE = 10, 3        # tensor 1 has no gradient for the first ADAM_LATE steps
ADAM_GROUPS = [dict(idx=[0, 1], lr=1e-4, betas=(0.9, 0.999), eps=1e-8), dict(idx=[2, 3], lr=5e-4, betas=(0.9, 0.999), eps=1e-8),
               dict(idx=[4], lr=5e-4, betas=(0.8, 0.99), eps=1e-6)]


@functools.lru_cache(maxsize=None)
def adam_inputs():
    """parameters and ADAM_STEPS gradients per tensor; each tensor's gradient magnitudes run over 1e-9 ... 10 element by
    element (an element keeps its magnitude over the steps), so that eps (1e-8, 1e-6) decides some updates and is invisible in others"""
    g = torch.Generator().manual_seed(5)
    ps = [torch.randn(n, generator=g) for n in ADAM_SIZES]
    mags = [10.0 ** (torch.rand(n, generator=g) * 10.0 - 9.0) if n > 1 else torch.tensor([1e-8]) for n in ADAM_SIZES]
    grads = [[torch.randn(n, generator=g) * mag for n, mag in zip(ADAM_SIZES, mags)] for it in range(ADAM_STEPS)]
    return ps, grads


def adam_lr(gi, it):
    return ADAM_GROUPS[gi]["lr"] * (1.0 - it / 20.0)


def adam_reference(dtype, eps_inside=False):
    """single-tensor Adam written out, operation by operation as torch.optim.Adam documents it -> parameters after
    ADAM_STEPS steps.  eps_inside: the wrong Adam that adds eps under the square root, sqrt(v / bc2 + eps) -- what the
    gradient magnitudes are chosen to tell apart (tests/test_layer_ref.py)"""
    ps, grads = adam_inputs()
    ps = [p.to(dtype).clone() for p in ps]
    m = [torch.zeros_like(p) for p in ps]
    v = [torch.zeros_like(p) for p in ps]
    step = [0] * len(ps)
    for it in range(ADAM_STEPS):
        for gi, grp in enumerate(ADAM_GROUPS):
            b1, b2 = grp["betas"]
            for i in grp["idx"]:
                if i == 1 and it < ADAM_LATE:
                    continue
                gr = grads[it][i].to(dtype)
                step[i] += 1
                m[i] = m[i] + (gr - m[i]) * (1.0 - b1)
                v[i] = v[i] * b2 + (1.0 - b2) * gr * gr
                bc1, bc2 = 1.0 - b1 ** step[i], 1.0 - b2 ** step[i]
                denom = (v[i] / bc2 + grp["eps"]).sqrt() if eps_inside else v[i].sqrt() / math.sqrt(bc2) + grp["eps"]
                ps[i] = ps[i] - (adam_lr(gi, it) / bc1) * (m[i] / denom)
    return ps


def adam_torch(dtype):
    """torch.optim.Adam itself on the same schedule"""
    ps, grads = adam_inputs()
    ps = [p.to(dtype).clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam([dict(params=[ps[i] for i in grp["idx"]], lr=grp["lr"], betas=grp["betas"], eps=grp["eps"])
                            for grp in ADAM_GROUPS], foreach=False)
    for it in range(ADAM_STEPS):
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = adam_lr(gi, it)
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and it < ADAM_LATE) else grads[it][i].to(dtype).clone()
        opt.step()
    return [p.detach() for p in ps]


# ------------------------------------------------------------------------------------------------------------------ #
# error measure and bound
# ------------------------------------------------------------------------------------------------------------------ #
def as2d(t):
    t = torch.as_tensor(t).detach().double().cpu()
    return t.reshape(-1, 1) if t.dim() < 2 else t.reshape(t.shape[0], -1)


SMALL_TILE = 32       # kept elements: at most one row or one column of a 32 x 32 tile


def tiles(got, r64, r32, tr, tc, floor=0.0, keep=None, floor_all=False):
    """-> [(row0, col0, err, e_ref, bound, max|ref|, floor applied)] per tr x tc tile (tc None: all columns), over the rows
    kept.  A floor counts only in a tile of at most SMALL_TILE kept elements, where e_ref is the largest of so few draws that
    it can sit far under an ulp; every larger tile is held to FACTOR e_ref alone.  floor_all: the one row whose floor is not
    about the tile's size (the chain's softplus, accurate in absolute terms by design)."""
    got, r64, r32 = as2d(got), as2d(r64), as2d(r32)
    assert got.shape == r64.shape == r32.shape, (got.shape, r64.shape, r32.shape)
    fl = as2d(floor) if torch.is_tensor(floor) else None       # an element-wise floor: the tile takes its largest
    assert fl is None or fl.shape == r64.shape
    R, C = r64.shape
    tc = tc or max(C, 1)
    out = []
    for r0 in range(0, R, tr):
        rows = torch.arange(r0, min(r0 + tr, R))
        if keep is not None:
            rows = rows[keep[rows]]
        if len(rows) == 0:
            continue
        for c0 in range(0, C, tc):
            a, b, c = got[rows, c0:c0 + tc], r64[rows, c0:c0 + tc], r32[rows, c0:c0 + tc]
            if b.numel() == 0:
                continue
            err, er, mx = float((a - b).abs().max()), float((c - b).abs().max()), float(b.abs().max())
            if not torch.isfinite(a).all():
                err = float("inf")
            f = 0.0
            if floor_all or b.numel() <= SMALL_TILE:
                f = float(fl[rows, c0:c0 + tc].max()) if fl is not None else float(floor)
            out.append((r0, c0, err, er, min(max(FACTOR * er, f), CAP * mx), mx, f))
    return out


def hold(case, name, got, r64, r32, tr, tc, rows_out, fails, floor=0.0, keep=None, e_ref_extra=None, floor_all=False):
    """the bound on every tile of one output; prints the worst tile, appends (case, output, worst err / e_ref, err, e_ref,
    bound, tiles, largest floor applied to a tile) to rows_out and the misses to fails.  e_ref_extra: further fp32 evaluations
    (operands permuted); a tile's e_ref is the worst of them all."""
    ts = tiles(got, r64, r32, tr, tc, floor, keep, floor_all)
    for extra in (e_ref_extra or []):
        ts = [(a[0], a[1], a[2], max(a[3], b[3]), max(a[4], b[4]), a[5], a[6])
              for a, b in zip(ts, tiles(got, r64, extra, tr, tc, floor, keep, floor_all))]
    worst = None
    for r0, c0, err, er, bd, mx, _ in ts:
        ratio = 0.0 if err == 0.0 else err / max(er, 1e-300)
        if worst is None or ratio > worst[0]:
            worst = (ratio, err, er, bd, r0, c0)
        if not err <= bd:
            fails.append("%s %s tile (%d, %d): err %.3e > bound %.3e (e_ref %.2e, max|ref| %.2e)" % (case, name, r0, c0, err, bd, er, mx))
    if worst is not None:
        print("%-34s %-8s tiles %3d worst err/e_ref %8.2f (err %.2e e_ref %.2e bound %.2e at %d,%d)"
              % (case, name, len(ts), worst[0], worst[1], worst[2], worst[3], worst[4], worst[5]))
        rows_out.append((case, name, worst[0], worst[1], worst[2], worst[3], len(ts), max(t[6] for t in ts)))
