"""The composite (udf -> occlusion / visibility -> two-sided alpha -> transmittance -> weighted sums) as a plain,
dtype-generic torch expression over the oracle's own functions, the generator of the inputs the composite matrix runs
on, and the error measures its bound is built from.  No GPU in here.

`oracle_composite` is the reference test_gpu_kernels.test_composite_stagewise used to carry inline; in float64 it is
the yardstick of tests/test_gpu_composite_matrix.py, in float32 it is the "other fp32 evaluation" that says how far a
correct fp32 implementation may sit from float64 on the same inputs (`e_ref`)."""
import functools

import torch

from oracle import udf_oracle as O

DIAG = ["alpha", "alpha_plus", "alpha_minus", "vis_prob", "alpha_occ", "raw_occ", "true_cos", "grad_mag", "mid_z",
        "dists", "inside", "flip"]
PER_SAMPLE_VALUES = ["weights"] + DIAG
PER_RAY_VALUES = ["color", "color_base", "depth", "normals", "wsum", "wsum_all", "sums"]
PER_SAMPLE_GRADS = ["d_udf", "d_grad", "d_color", "d_color_base", "d_bg_sigma", "d_bg_color"]
BATCH_GRADS = ["d_inv_s", "d_beta", "d_gamma"]
EXACT = ("inside", "flip")
VALUE_FLOOR, GRAD_FLOOR, FACTOR, CAP = 1e-5, 1e-4, 4.0, 1e-3
MARGIN = 1e-5


def oracle_composite(geom, u, gr, c, b, s_, be, ga, bs=None, bc=None, *, kind="numerical", anneal=None, fs=0.0,
                     use_norm=False, background_rgb=None, s_nominal=None, sparse_scale=25000.0):
    """geom: rays_o [N,3], rays_d [N,3], z [N,S], sdist (float), bg_z [N,n_out] or None -- taken in u's dtype.
    u [N,S], gr [N,S,3], c / b [N,S,3] (colour, base colour), s_ / be / ga [1] (inv_s, beta, gamma), bs [N,n_out],
    bc [N,n_out,3].  -> every output of the composite launch and its twelve diagnostic arrays."""
    dt = u.dtype
    z, ro, rd = geom["z"].to(dt), geom["rays_o"].to(dt), geom["rays_d"].to(dt)
    sdist = float(geom["sdist"])
    N, S = z.shape
    one = torch.ones(N, 1, dtype=dt)
    dists = torch.cat([z[:, 1:] - z[:, :-1], sdist * one], -1)
    mid = z + dists * 0.5
    dirs = rd[:, None, :].expand(N, S, 3)
    pts = ro[:, None, :] + dirs * mid[..., None]
    gm = torch.linalg.norm(gr, ord=2, dim=-1, keepdim=True)
    gn = gr / (gm + 1e-5)
    tc = (dirs * (gn if use_norm else gr)).sum(-1)
    flip = -torch.sign((dirs * gn).sum(-1))
    flip[flip == 0] = 1
    flip = flip.detach()
    raw = O.udf2logistic(u, be, 1.0, 1.0)
    aocc = 1.0 - torch.exp(-torch.relu(raw) * ga * dists)
    vm = torch.cat([(tc < 0.01).to(dt)[:, 1:], one], -1)
    vis = O.excl_cumprod((1.0 - aocc + fs * vm).clip(0, 1) + 1e-7).clip(0, 1)
    ap = O.sdf2alpha(u, -tc.abs(), dists, s_, anneal, kind=kind)
    am = O.sdf2alpha(-u, -tc.abs(), dists, s_, anneal, kind=kind)
    alpha = ap * vis + am * (1 - vis)
    alpha_in = alpha
    cc, bb = c, b
    if bs is not None:
        bg_z = geom["bg_z"].to(dt)
        dz = torch.cat([bg_z[:, 1:] - bg_z[:, :-1], sdist * one], -1)
        alpha = torch.cat([alpha, 1.0 - torch.exp(-torch.relu(bs) * dz)], -1)
        cc = torch.cat([c, bc], 1)
        bb = torch.cat([b, bc], 1)
    w = alpha * O.excl_cumprod(1.0 - alpha + 1e-7)
    pn = torch.linalg.norm(pts, ord=2, dim=-1)
    ge = (gm[..., 0] - 1.0) ** 2
    relax, near = (pn < 1.2).to(dt), (u < 0.05).to(dt).detach()
    sums = torch.stack([(relax * ge).sum(), relax.sum(), (near * ge).sum(), near.sum(),
                        torch.exp(-sparse_scale * u).sum()])
    wsum_all = w.sum(-1, keepdim=True)
    color = (cc * w[..., None]).sum(1)
    if background_rgb is not None:
        color = color + background_rgb.to(dt) * (1.0 - wsum_all)
    sn = S if s_nominal is None else min(int(s_nominal), w.shape[1])
    return dict(color=color, color_base=(bb * w[..., None]).sum(1), weights=w,
                depth=(mid * w[:, :S]).sum(1, keepdim=True), normals=(flip[..., None] * gr * w[:, :S, None]).sum(1),
                sums=sums, wsum=w[:, :sn].sum(-1, keepdim=True), wsum_all=wsum_all,
                vis=vis, vis_prob=vis, alpha=alpha_in, alpha_plus=ap, alpha_minus=am, alpha_occ=aocc, raw_occ=raw,
                true_cos=tc, grad_mag=gm[..., 0], mid_z=mid, dists=dists, inside=(pn < 1.0).to(dt), flip=flip,
                _pn=pn, _cos_n=(dirs * gn).sum(-1), _tc_raw=(dirs * gr).sum(-1), _tc_norm=(dirs * gn).sum(-1))


# ------------------------------------------------------------------------------------------------------------------ #
# the matrix: (S, n_out, s_nominal) and the renderer settings rotated over it
# ------------------------------------------------------------------------------------------------------------------ #
SHAPES = [(1, 0), (2, 0), (64, 0), (63, 1),                      # nc 1
          (65, 0), (128, 0),                                     # nc 2
          (128, 9), (100, 33), (192, 0),                         # nc 3
          (256, 0), (250, 0),                                    # nc 4
          (320, 0), (300, 7),                                    # nc 5
          (384, 0), (350, 20),                                   # nc 6 (the ragged one is this file's addition)
          (385, 0), (352, 33), (448, 0), (400, 33),              # nc 7 -> <8>, one dead chunk
          (449, 0), (512, 0), (479, 33)]                         # nc 8
NOMINAL = [(128, 0, 100), (256, 0, 192), (250, 0, 240), (449, 0, 400)]
_ANNEAL, _FS = [None, 0.0, 0.6, 1.0], [0.0, 0.9, 1.0]


def n_chunks(S, n_out):
    return (S + n_out + 63) // 64


def _settings(i):
    return dict(cos_anneal=_ANNEAL[i % 4], use_norm_grad=(i // 3) % 2 == 1, alpha_type=(i // 2) % 2,
                flip_saturation=_FS[i % 3], background=(i % 5) in (1, 3))


# base seeds: the first seed of a search from 100 + 200 i at which the case meets the threshold margins of `make_case`
# and the conditions of `degenerate` (found on the CPU, without a kernel)
_SEEDS = [100, 301, 501, 700, 901, 1100, 1300, 1500, 1703, 1901, 2100, 2304, 2508, 2710, 2902, 3116, 3301, 3501, 3701,
          3914, 4122, 4302, 4500, 4700, 4900, 5109]
CASES = []
for _i, (_S, _no, _sn) in enumerate([(s, o, s) for s, o in SHAPES] + NOMINAL):
    CASES.append(dict(S=_S, n_out=_no, s_nominal=_sn, seed=_SEEDS[_i], **_settings(_i)))


def case_id(c):
    return "S%d_out%d_nom%d" % (c["S"], c["n_out"], c["s_nominal"])


def instantiation(S, n_out, s_nominal, diagnostics):
    """the kernels nudf_composite_fwd / _bwd launch for a shape (the dispatch conditions at the end of composite.hip)"""
    nc = n_chunks(S, n_out)
    NC = nc if nc <= 6 else 8
    full = S == 64 * NC and n_out == 0 and s_nominal >= S
    fwd = "composite_fwd_kernel<%d, %s>" % (NC, "DIAG" if diagnostics else ("FULL" if full else "plain"))
    return fwd, "composite_bwd_kernel<%d, %s>" % (NC, "FULL" if full else "ragged")


# ------------------------------------------------------------------------------------------------------------------ #
# inputs
# ------------------------------------------------------------------------------------------------------------------ #
def _draw(S, n_out, seed, n_rays):
    g = torch.Generator().manual_seed(seed)
    ST = S + n_out
    nc = n_chunks(S, n_out)
    N = 2 * (nc + 1) + 1 if n_rays is None else n_rays
    span = 2.0 * min(1.0, 48.0 / ST)
    sdist = 0.01
    # rays through the unit sphere: the sample at depth z sits at radius ~ |z - t| (+ a small lateral offset), t spread
    # so that the 1.0 and 1.2 spheres are crossed inside the sampled span on part of the rays
    rd = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    lat = torch.nn.functional.normalize(torch.cross(rd, torch.randn(N, 3, generator=g), dim=-1), dim=-1)
    t = torch.linspace(-0.25, 0.15, N)[torch.randperm(N, generator=g)] if N > 1 else torch.zeros(1)
    ro = -rd * t[:, None] + lat * 0.1
    z = 1.0 + span * (torch.arange(S)[None, :] + torch.rand(N, S, generator=g)) / S
    level = torch.linspace(0.04, 0.16, N)[torch.randperm(N, generator=g)]
    udf = level[:, None] * (0.6 + 0.8 * torch.rand(N, S, generator=g))
    lane = torch.randint(0, 64, (N,), generator=g)
    for r in range(N):
        k = r % (nc + 1)                        # pattern nc: no dip
        lo, hi = 64 * k, min(64 * k + 64, S)
        if k < nc and lo < hi:
            udf[r, lo + int(lane[r]) % (hi - lo)] = 1e-4 * (1 + r % 19)
    grad = torch.randn(N, S, 3, generator=g) * 0.8
    col = torch.rand(N, S, 3, generator=g)
    cb = torch.rand(N, S, 3, generator=g)
    out = dict(N=N, S=S, n_out=n_out, rays_o=ro, rays_d=rd, z=z, sdist=sdist, udf=udf, grad=grad, color=col,
               color_base=cb, inv_s=torch.tensor([30.0]), beta=torch.tensor([60.0]), gamma=torch.tensor([20.0]),
               bg_z=None, bg_sigma=None, bg_color=None, background_rgb=torch.rand(3, generator=g))
    if n_out:
        out["bg_z"] = z[:, -1:] + 0.2 + 0.05 * (torch.arange(n_out)[None, :] + torch.rand(N, n_out, generator=g))
        out["bg_sigma"] = torch.randn(N, n_out, generator=g) * 0.5
        out["bg_color"] = torch.rand(N, n_out, 3, generator=g)
    # the fixed random linear functional of all outputs whose gradient the backward is held against
    out["wts"] = dict(color=torch.randn(N, 3, generator=g), color_base=torch.randn(N, 3, generator=g),
                      weights=torch.randn(N, ST, generator=g) * 0.1, depth=torch.randn(N, 1, generator=g),
                      normals=torch.randn(N, 3, generator=g), wsum=torch.randn(N, 1, generator=g),
                      wsum_all=torch.randn(N, 1, generator=g),
                      sums=torch.tensor([0.02, 0.003, 0.01, -0.002, 2e-4]))
    return out


def _ray_margins(inp):
    """per ray, the smallest distance of any of its samples from each threshold the kernels branch on (float64)"""
    z = inp["z"].double()
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((z.shape[0], 1), inp["sdist"], dtype=torch.float64)], -1)
    mid = z + 0.5 * dists
    rd = inp["rays_d"].double()
    pts = inp["rays_o"].double()[:, None, :] + rd[:, None, :] * mid[..., None]
    pn = pts.norm(dim=-1)
    gr = inp["grad"].double()
    gn = gr / (gr.norm(dim=-1, keepdim=True) + 1e-5)
    tc_raw, cn = (rd[:, None, :] * gr).sum(-1), (rd[:, None, :] * gn).sum(-1)
    m = lambda t: t.min(dim=1)[0]
    return dict(true_cos=m(torch.minimum((tc_raw - 0.01).abs(), (cn - 0.01).abs())), relax=m((pn - 1.2).abs()),
                inside=m((pn - 1.0).abs()), near=m((inp["udf"].double() - 0.05).abs()), flip=m(cn.abs()))


def margins(inp):
    """smallest distance of any sample from each threshold: |true_cos - 0.01| (both forms of true_cos), | |p| - 1.2 |,
    | |p| - 1.0 |, |udf - 0.05|, |cos_n|"""
    return {k: float(v.min()) for k, v in _ray_margins(inp).items()}


@functools.lru_cache(maxsize=None)
def make_case(S, n_out, seed, n_rays=None):
    """fp32 inputs of one case: the first of the seeds seed, seed + 1, ... (20 at the most) whose samples all keep MARGIN
    from every threshold the kernels branch on, so that no fp32 implementation can legitimately select differently.
    With `n_rays` (thousands of rays: no whole draw qualifies) the same search runs per ray: a ray that fails takes its
    row from the next seed's draw."""
    if n_rays is None:
        for k in range(20):
            inp = _draw(S, n_out, seed + k, None)
            if min(margins(inp).values()) >= MARGIN:
                inp["seed_used"] = seed + k
                return inp
        raise AssertionError("degenerate inputs: no seed in %d..%d keeps %g from every threshold" % (seed, seed + 19, MARGIN))
    inp = _draw(S, n_out, seed, n_rays)
    for k in range(1, 20):
        bad = torch.stack(list(_ray_margins(inp).values())).min(dim=0)[0] < MARGIN
        if not bool(bad.any()):
            inp["seed_used"] = seed + k - 1
            return inp
        nxt = _draw(S, n_out, seed + k, n_rays)
        for d, e in ((inp, nxt), (inp["wts"], nxt["wts"])):
            for key, t in d.items():
                if isinstance(t, torch.Tensor) and t.dim() >= 2 and t.shape[0] == n_rays:
                    t[bad] = e[key][bad]
    raise AssertionError("degenerate inputs: rays left within %g of a threshold after 20 draws" % MARGIN)


# ------------------------------------------------------------------------------------------------------------------ #
# evaluation: outputs + gradients of the linear functional, in a dtype
# ------------------------------------------------------------------------------------------------------------------ #
def functional(o, wts, to=lambda t: t):
    return sum((o[k] * to(wts[k])).sum() for k in wts)


def evaluate(inp, cfg, dtype, scalar_params=None):
    """-> (outputs, gradients) of oracle_composite in `dtype`, detached.  `scalar_params` = (variance, beta, gamma,
    beta_hi): the three scalars are formed from the 1-element parameters as the scalar networks form them
    (exp(10 p) + the clips) and d_param holds the gradients w.r.t. the parameters."""
    L = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    lv = dict(udf=L(inp["udf"]), grad=L(inp["grad"]), color=L(inp["color"]), color_base=L(inp["color_base"]),
              inv_s=L(inp["inv_s"]), beta=L(inp["beta"]), gamma=L(inp["gamma"]), bg_sigma=L(inp["bg_sigma"]),
              bg_color=L(inp["bg_color"]))
    s_, be, ga = lv["inv_s"], lv["beta"], lv["gamma"]
    pl = None
    if scalar_params is not None:
        pl = [L(p) for p in scalar_params[:3]]
        s_ = torch.exp(10.0 * pl[0]).clip(1e-6, 1e6)
        be = torch.exp(10.0 * pl[1]).clip(0, float(scalar_params[3])).clip(1e-6, 1e6)
        ga = torch.exp(10.0 * pl[2]).clip(1e-6, 1e6)
    bgc = cfg.get("background_rgb")
    o = oracle_composite(inp, lv["udf"], lv["grad"], lv["color"], lv["color_base"], s_, be, ga, lv["bg_sigma"],
                         lv["bg_color"], kind="theorical" if cfg["alpha_type"] else "numerical", anneal=cfg["cos_anneal"],
                         fs=cfg["flip_saturation"], use_norm=cfg["use_norm_grad"], background_rgb=bgc,
                         s_nominal=cfg["s_nominal"], sparse_scale=cfg.get("sparse_scale", 25000.0))
    functional(o, inp["wts"], lambda t: t.to(dtype)).backward()
    G = lambda t: None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad.detach())
    grads = dict(d_udf=G(lv["udf"]), d_grad=G(lv["grad"]), d_color=G(lv["color"]), d_color_base=G(lv["color_base"]),
                 d_bg_sigma=G(lv["bg_sigma"]), d_bg_color=G(lv["bg_color"]))
    if pl is None:
        grads.update(d_inv_s=G(lv["inv_s"]), d_beta=G(lv["beta"]), d_gamma=G(lv["gamma"]))
    else:
        grads["d_param"] = torch.cat([G(p).reshape(1) for p in pl])
    return {k: v.detach() for k, v in o.items()}, grads


def case_cfg(c, inp):
    return dict(s_nominal=c["s_nominal"], cos_anneal=c["cos_anneal"], flip_saturation=c["flip_saturation"],
                use_norm_grad=c["use_norm_grad"], alpha_type=c["alpha_type"], sparse_scale=25000.0,
                background_rgb=inp["background_rgb"] if c["background"] else None)


@functools.lru_cache(maxsize=None)
def reference(idx):
    """(inputs, cfg, float64 outputs, float64 gradients, fp32 outputs, fp32 gradients) of CASES[idx]; computed once and
    shared by every test of the case -- callers leave the tensors unchanged"""
    c = CASES[idx]
    inp = make_case(c["S"], c["n_out"], c["seed"])
    cfg = case_cfg(c, inp)
    o64, g64 = evaluate(inp, cfg, torch.float64)
    o32, g32 = evaluate(inp, cfg, torch.float32)
    return inp, cfg, o64, g64, o32, g32


# ------------------------------------------------------------------------------------------------------------------ #
# error measures and the bound
# ------------------------------------------------------------------------------------------------------------------ #
def chunk_errors(a, b, offset=0):
    """true relative error max|a - b| / max|b| of every 64-sample chunk of dim 1 (chunk = (offset + index) // 64, the
    lane layout of the kernels) -> list of (chunk, error, max|b|)"""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    out = []
    n = a.shape[1]
    i = 0
    while i < n:
        k = (offset + i) // 64
        j = min(n, 64 * (k + 1) - offset)
        d, m = float((a[:, i:j] - b[:, i:j]).abs().max()), float(b[:, i:j].abs().max())
        out.append((k, 0.0 if d == 0.0 else d / max(m, 1e-300), m))
        i = j
    return out


def tensor_error(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    d = float((a - b).abs().max())
    return 0.0 if d == 0.0 else d / max(float(b.abs().max()), 1e-300)


def error(name, a, b, S):
    """the issue's measure of one tensor: worst 64-sample chunk for per-sample tensors, whole tensor otherwise"""
    if name in PER_SAMPLE_VALUES or name in PER_SAMPLE_GRADS:
        off = S if name in ("d_bg_sigma", "d_bg_color") else 0
        return max(e for _, e, _ in chunk_errors(a, b, off))
    return tensor_error(a, b)


def floor_of(name):
    return GRAD_FLOOR if name.startswith("d_") else VALUE_FLOOR


def bound(name, e_ref):
    """max(4 e_ref, floor) capped at 1e-3: e_ref = the fp32 torch evaluation's own distance from float64 for that case
    and tensor.  Kernel and fp32 torch are two independent fp32 evaluations: the kernel's v_exp / v_rcp / v_sqrt are
    <= 1 ulp where torch's are 0.5 ... 1 ulp, and its scans associate in log depth where torch's are serial."""
    return min(max(FACTOR * e_ref, floor_of(name)), CAP)


def ratio(name, e_kernel, e_ref):
    return e_kernel / max(e_ref, floor_of(name) / FACTOR)


def degenerate(inp, cfg, o64, g64):
    """the conditions a case must meet to say anything about a late chunk -> list of violations (empty = fine)"""
    S, n_out = inp["S"], inp["n_out"]
    bad = []
    for nm, t in (("weights", o64["weights"]), ("d_udf", g64["d_udf"]), ("d_grad", g64["d_grad"]),
                  ("d_color", g64["d_color"])):
        ce = chunk_errors(t, t)
        top = max(m for _, _, m in ce)
        for k, _, m in ce:
            if not m >= 1e-3 * top:
                bad.append("%s: chunk %d holds %.2e of the tensor's max" % (nm, k, m / top))
    # the three batch gradients are sums over all samples: where one of them cancels to nothing (two samples per ray and
    # a saturated visibility clip leave d beta ~ 1e-15) a relative error says nothing about it
    for nm in BATCH_GRADS:
        if S > 1 and nm in g64 and not abs(float(g64[nm])) >= 1e-4:
            bad.append("%s = %.2e: cancels to nothing" % (nm, float(g64[nm])))
    if S > 2:
        v = o64["vis_prob"]
        for k in range((S + 63) // 64):
            blk = v[:, 64 * k:min(S, 64 * k + 64)]
            n = int(((blk > 0.05) & (blk < 0.95)).any(dim=1).sum())
            if n < 2:
                bad.append("vis_prob: chunk %d has %d rays with a visibility in (0.05, 0.95)" % (k, n))
    return bad


# ------------------------------------------------------------------------------------------------------------------ #
# up-sampler inputs
# ------------------------------------------------------------------------------------------------------------------ #
UP_M = [64, 65, 129, 192, 256, 257, 320, 449, 511, 512]                # 64 and 256 added: <1> and <4> need them
UP_SETTINGS = [(16, 64.0, 40.0, 20.0), (1, 256.0, 80.0, 20.0)]        # K, inv_s, beta, gamma
UP_N = 37


@functools.lru_cache(maxsize=None)
def make_upsample_case(M, late=False):
    """synthetic (z, udf) of one up-sampling round: a surface at z_s in [1, 2.2] per ray, the second half of the rays
    grazing.  z reaches 2.6, so a hit at z_s <= 2.2 leaves the last eighth of a long ray (its last chunk) without new
    samples: `late` draws z_s in [2.2, 2.55] instead, and every shape runs on both."""
    g = torch.Generator().manual_seed(7000 + 13 * M + (5000 if late else 0))
    N = UP_N
    z = torch.sort(0.6 + 2.0 * torch.rand(N, M, generator=g), -1)[0]
    zs = (2.2 + 0.35 * torch.rand(N, 1, generator=g)) if late else (1.0 + 1.2 * torch.rand(N, 1, generator=g))
    slope = 0.3 + 0.6 * torch.rand(N, 1, generator=g)
    udf = (z - zs).abs() * slope + 0.002 * torch.rand(N, M, generator=g)
    udf[N // 2:] += 0.05                                                # grazing rays: no hit
    rd = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    lat = torch.nn.functional.normalize(torch.cross(rd, torch.randn(N, 3, generator=g), dim=-1), dim=-1)
    ro = -rd * 1.6 + lat * (0.6 * torch.rand(N, 1, generator=g))        # the unit sphere spans z in ~[0.6, 2.6]
    return dict(N=N, M=M, z=z.contiguous(), udf=udf.contiguous(), rays_o=ro.contiguous(), rays_d=rd.contiguous(),
                sdist=2.0 / 64)


def oracle_upsample(inp, mode, K, inv_s, beta, gamma, dtype):
    """the oracle's up-sampling round in `dtype` (its constants follow torch's default dtype, switched for the call)"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        z, udf = inp["z"].to(dtype), inp["udf"].to(dtype)
        if mode == 1:
            return O.up_sample_no_occ_aware(z, udf, inp["sdist"], K, beta, gamma)
        return O.up_sample_unbias(inp["rays_o"].to(dtype), inp["rays_d"].to(dtype), z, udf, inp["sdist"], K, inv_s, beta,
                                  gamma)
    finally:
        torch.set_default_dtype(old)


def last_section_chunk(M):
    """chunk of the last of the M - 1 sections of a ray"""
    return (M - 2) // 64


def quantile_chunks(inp, z_new):
    """the 64-sample chunks of z the new samples of a round fall into (any ray) -> sorted list"""
    idx = torch.searchsorted(inp["z"].double().contiguous(), z_new.double().contiguous(), right=True) - 1
    return sorted(set((idx.clamp(min=0) // 64).flatten().tolist()))
