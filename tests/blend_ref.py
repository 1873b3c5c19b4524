"""The image-based blending branch (pixel warp -> view softmax -> inside / background mix -> weighted sums; patch warp ->
per-view usability -> view softmax -> weighted sum) as the oracle's own functions in a caller-chosen dtype, the generator
of the inputs the blend matrix runs on, the margins of the discrete decisions the kernels take, and the error measures
its bound is built from.  No GPU in here, `launch` (the call under test) aside.

`evaluate(inp, float64)` is the yardstick of tests/test_gpu_blend_matrix.py and of test_gpu_blend.test_blend_stagewise;
`evaluate(inp, float32)` is the "other fp32 evaluation" that says how far a correct fp32 implementation may sit from
float64 on the same inputs (`e_ref`).  Inputs are drawn in float32 and cast, so both precisions and the GPU see the same
numbers; the float64 side builds its camera constants in float64 from the same fp32 poses and intrinsics, the fp32 side
(like models/blend.py) from fp32 `torch.inverse` -- that difference is part of e_ref.

Ties.  O.pixel_warp / O.patch_warp do not return the quantities their masks threshold, so `geometry` restates them (the
per-element form of csrc/blend.hip) and tests/test_blend_ref.py pins its masks to the oracle's.  A decision is robust when
its float64 quantity keeps MARGIN (unit-less quantities) or PIX_MARGIN (source-image pixel coordinates) from the
threshold; a ray -- or, for the per-view warps, a (sample, view) or a patch pixel -- with a decision that is not robust is
left out of the comparison, and a case may leave out no more than RAY_TIE_CAP of its rays (PIXEL_TIE_CAP of its patch
pixels)."""
import contextlib
import functools

import torch

from common import smooth_images
from composite_ref import CAP, FACTOR, GRAD_FLOOR, MARGIN, VALUE_FLOOR, tensor_error
from neuraludf_amd import synth
from oracle import udf_oracle as O

# Source-image coordinates reach W = 128: one fp32 ulp there is 7.6e-6 px, and a coordinate is the quotient of two sums of
# three products of a chain of three 3x3 matrix products (K_src (R + t n^T / d) K_ref^-1, entries up to ~250): some tens of
# roundings at that magnitude.  1e-3 px = 130 ulp(128) covers a well-conditioned homography; an ill-conditioned one gets a
# margin of its own (pixel_margin).  tests/test_blend_ref.py asserts that no fp32 / float64 decision differs outside the
# margins.
PIX_MARGIN = 1e-3
MOVE_FACTOR = 8.0                # see pixel_margin
RAY_TIE_CAP, PIXEL_TIE_CAP = 0.10, 1e-3
VALUES = ["color_pixel", "patch_colors", "patch_mask"]
GRADS = ["d_logits", "d_w", "d_bg_in", "d_bg_tail"]
N_REF = 128                      # rays of the float64 reference of a 1024-ray case (ray 0 and ray N - 1 among them)


@contextlib.contextmanager
def default_dtype(dtype):
    """the oracle's warps are dtype-generic except for a few constants that follow torch's default dtype (torch.ones, the
    z axis; the fp32 integer patch offsets promote exactly); switched for the block and restored whatever happens inside"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------------------------ #
# the matrix
# ------------------------------------------------------------------------------------------------------------------ #
# bg: "both" = bg_in [N,S,3] and bg_tail [N,n_out,3], "in" = bg_in alone (n_out = 0), "tail" = bg_tail alone, None.
# hps None = composite-only rows (rays_uv=None: pixel_blend + pixel_composite, no patch launch).
def _case(hps, N, S, V, nl, n_out, bg, seed, reaches):
    return dict(hps=hps, N=N, S=S, V=V, nl=nl, n_out=n_out, bg=bg, seed=seed, reaches=reaches)


CASES = [
    _case(1, 9, 3, 8, 10, 0, None, 101, "<.,1,8>; S < waves: idle waves in the LDS sum"),
    _case(2, 33, 64, 8, 8, 0, "in", 202, "<.,1,8>; nl == V; S a multiple of the wave count; S + n_out = 64"),
    _case(3, 21, 37, 8, 10, 5, "both", 301, "<.,1,8>; ldw > S; S + n_out = 42"),
    _case(4, 70, 13, 3, 10, 0, None, 401, "<.,2,8>; 17 live lanes in chunk 1; V < 8"),
    _case(5, 21, 37, 8, 10, 5, "both", 501, "<.,2,8>; the shipped fine-tune patch size"),
    _case(5, 1024, 7, 8, 10, 0, None, 601, "<.,2,4>; S not a multiple of 4; N % 4 == 0"),
    _case(3, 1024, 7, 10, 10, 0, "in", 701, "<.,1,4>; V = MAXV = nl"),
    _case(None, 10, 64, 8, 10, 5, "tail", 801, "composite only: S + n_out = 69, a 5-lane second pass"),
    _case(None, 7, 100, 8, 10, 33, "both", 901, "composite only: S + n_out = 133, a third pass"),
    _case(None, 8, 37, 5, 10, 5, "tail", 1001, "composite only: S + n_out = 42, N % 4 == 0, V < 8"),
]
CASES.append(_case(3, 21, 37, 8, 10, 0, None, 1101, "<.,1,8>; the stage-wise test's shape without a background"))
STAGEWISE = {True: 2, False: len(CASES) - 1}      # test_gpu_blend.test_blend_stagewise[with_bg]


def case_id(c):
    return "hps%s_N%d_S%d_V%d_nl%d_out%d_bg%s" % (c["hps"], c["N"], c["S"], c["V"], c["nl"], c["n_out"], c["bg"])


def instantiations(c):
    """the kernels blend_and_composite launches for a case (the dispatch of csrc/blend.hip), forward and backward"""
    k = ["pixel_blend_kernel<false>", "pixel_blend_kernel<true>", "pixel_composite_kernel<false>",
         "pixel_composite_kernel<true>"]
    if c["hps"] is not None:
        pc = 2 if (2 * c["hps"] + 1) ** 2 > 64 else 1
        wv = 4 if c["N"] >= 1024 else 8
        k += ["patch_blend_kernel<false,%d,%d>" % (pc, wv), "patch_blend_kernel<true,%d,%d>" % (pc, wv)]
    return k


# the per-view warps behind PatchProjector: N x S not a multiple of 4, both PC
WARP_CASES = [dict(hps=3, N=19, S=23, V=8, seed=1403), dict(hps=5, N=19, S=23, V=8, seed=1505)]


# ------------------------------------------------------------------------------------------------------------------ #
# inputs
# ------------------------------------------------------------------------------------------------------------------ #
def npx_of(hps):
    return (2 * hps + 1) ** 2


def _scene_inputs(N, S, V, hps, seed, g):
    scene = synth.make_scene("tiny")
    r = synth.make_rays(scene, 0, N, seed=seed, margin=max(4, 2 * (hps or 0)))
    src = synth.make_source_views(scene, 0, V)
    # depths from 0.3 before the unit sphere to 0.3 behind it: |z - mid| <= 1.3 while the sphere ends at sqrt(1 - b^2) <= 1
    # (b the ray's distance from the origin), so 23 % of the samples and more lie outside
    lo, hi = r["near"] - 0.3, r["far"] + 0.3
    z = torch.sort(lo + (hi - lo) * torch.rand(N, S, generator=g), -1)[0]
    pts = (r["rays_o"][:, None] + r["rays_d"][:, None] * z[..., None]).contiguous()
    return dict(N=N, S=S, V=V, hps=hps, H=scene.H, W=scene.W, pts=pts, rays_d=r["rays_d"], rays_uv=r["rays_uv"],
                imgs=smooth_images(V, scene.H, scene.W), intrinsics=src["intrinsics"], w2cs=src["w2cs"],
                src_c2ws=src["src_c2ws"], query_c2w=src["query_c2w"])


@functools.lru_cache(maxsize=None)
def make_case(idx):
    """fp32 inputs of CASES[idx] (shared: callers leave the tensors unchanged)"""
    c = CASES[idx]
    N, S, V, nl, n_out, hps = c["N"], c["S"], c["V"], c["nl"], c["n_out"], c["hps"]
    g = torch.Generator().manual_seed(c["seed"])
    inp = _scene_inputs(N, S, V, hps, c["seed"], g)
    inp.update(nl=nl, n_out=n_out, grad=torch.randn(N, S, 3, generator=g), logits=torch.randn(N, S, nl, generator=g),
               w=torch.rand(N, S + n_out, generator=g) * 0.05,
               bg_in=torch.rand(N, S, 3, generator=g) if c["bg"] in ("both", "in") else None,
               bg_tail=torch.rand(N, n_out, 3, generator=g) if c["bg"] in ("both", "tail") else None,
               k1=torch.randn(N, 3, generator=g),
               k2=torch.randn(N, npx_of(hps), 3, generator=g) if hps is not None else None)
    assert (inp["bg_tail"] is not None) == (n_out > 0)
    return inp


@functools.lru_cache(maxsize=None)
def make_warp_case(idx):
    c = WARP_CASES[idx]
    g = torch.Generator().manual_seed(c["seed"])
    inp = _scene_inputs(c["N"], c["S"], c["V"], c["hps"], c["seed"], g)
    inp["normals"] = torch.nn.functional.normalize(torch.randn(c["N"], c["S"], 3, generator=g), dim=-1)
    return inp


_PER_RAY = ("pts", "rays_d", "rays_uv", "grad", "logits", "w", "bg_in", "bg_tail", "k1", "k2", "normals")


def ref_rays(N):
    """the rays a case's reference is evaluated on: all of them, or N_REF spread over a 1024-ray case, both ends included"""
    if N <= 2 * N_REF:
        return torch.arange(N)
    return torch.unique(torch.linspace(0, N - 1, N_REF).round().long())


def take_rays(inp, rows):
    out = dict(inp)
    for k in _PER_RAY:
        if out.get(k) is not None:
            out[k] = out[k][rows].contiguous()
    out["N"] = len(rows)
    return out


def cameras(inp, dtype):
    """(intrinsics, w2cs, src_c2ws, query_c2w) in `dtype`.  fp32: what models/blend.py is handed and forms (the fp32 w2cs,
    their fp32 inverse as the source poses); float64: from the fp32 poses themselves, inverted in float64."""
    if dtype == torch.float32:
        return inp["intrinsics"], inp["w2cs"], torch.inverse(inp["w2cs"]), inp["query_c2w"]
    c2w = inp["src_c2ws"].to(dtype)
    return inp["intrinsics"].to(dtype), torch.inverse(c2w), c2w, inp["query_c2w"].to(dtype)


# ------------------------------------------------------------------------------------------------------------------ #
# reference
# ------------------------------------------------------------------------------------------------------------------ #
def color_blend(logits, pix_col, pix_mask, patch_col=None, patch_mask=None):
    """O.color_blend with its two `.float()` casts of the normalising sums taken out: they are no-ops in fp32 (this
    function and the oracle's then agree bit for bit, tests/test_blend_ref.py) and would round the float64 reference's
    denominators to fp32."""
    v = pix_col.shape[-2]
    x = logits[:, :, :v]
    w = torch.softmax(x, -1) * pix_mask
    w = w / (w.sum(-1, keepdim=True) + 1e-8)
    pix = (pix_col * w[:, :, :, None]).sum(-2)
    pcol = pm = None
    if patch_col is not None:
        npx = patch_col.shape[3]
        vm = patch_mask.sum(-1) > npx - 1
        w2 = torch.softmax(x, -1) * vm
        w2 = w2 / (w2.sum(-1, keepdim=True) + 1e-8)
        pcol = (patch_col * w2[:, :, :, None, None]).sum(-3)
        pm = vm.sum(-1, keepdim=True) > 0
    return pix, pcol, pm


def flipped_normals(inp, dtype):
    """normals = -sign(rays_d . g) g with g = grad / (|grad| + 1e-5), sign(0) -> 1 (udf_renderer_blending.py:447)"""
    grad, rd = inp["grad"].to(dtype), inp["rays_d"].to(dtype)
    gn = grad / (torch.linalg.norm(grad, dim=-1, keepdim=True) + 1e-5)
    flip = -torch.sign((rd[:, None] * gn).sum(-1, keepdim=True))
    flip[flip == 0] = 1
    return flip * gn


def evaluate(inp, dtype):
    """-> (values, gradients, masks) of the blending branch in `dtype`, detached.  values: color_pixel [N,3],
    patch_colors [N,Npx,3], patch_mask [N]; gradients of sum(color_pixel k1) + sum(patch_colors k2): d_logits [N,S,nl],
    d_w [N,S+n_out], d_bg_in, d_bg_tail; masks: pix [N,S,V], patch [N,S,V,Npx], inside [N,S] (bool)."""
    N, S, hps = inp["N"], inp["S"], inp["hps"]
    with default_dtype(dtype):
        intr, w2cs, c2ws, qc2w = cameras(inp, dtype)
        L = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
        lg, w, bg_in, bg_tail = L(inp["logits"]), L(inp["w"]), L(inp["bg_in"]), L(inp["bg_tail"])
        pts, imgs = inp["pts"].to(dtype), inp["imgs"].to(dtype)
        pcol, pmask = O.pixel_warp(pts, imgs, intr, w2cs)
        tcol = tmask = None
        if hps is not None:
            tcol, tmask = O.patch_warp(pts, inp["rays_uv"].to(dtype), flipped_normals(inp, dtype), imgs, intr[0], intr,
                                       qc2w, c2ws, hps)
        pix, patch, pm = color_blend(lg, pcol, pmask, tcol, tmask)
        inside = torch.linalg.norm(pts, dim=-1) < 1.0
        if bg_in is not None:                                     # udf_renderer_blending.py:503-506
            ins = inside.to(dtype)[..., None]
            pix = pix * ins + bg_in * (1 - ins)
        if bg_tail is not None:
            pix = torch.cat([pix, bg_tail], 1)
        vals = dict(color_pixel=(pix * w[:, :, None]).sum(1))
        f = (vals["color_pixel"] * inp["k1"].to(dtype)).sum()
        if hps is not None:
            vals["patch_colors"] = (patch * w[:, :S, None, None]).sum(1)
            vals["patch_mask"] = (pm.to(dtype).reshape(N, S) * w[:, :S]).sum(1)
            f = f + (vals["patch_colors"] * inp["k2"].to(dtype)).sum()
        f.backward()
        G = lambda t: None if t is None else t.grad.detach()
        grads = dict(d_logits=G(lg), d_w=G(w), d_bg_in=G(bg_in), d_bg_tail=G(bg_tail))
        masks = dict(pix=pmask.bool(), patch=None if tmask is None else tmask.bool(), inside=inside)
    return {k: v.detach() for k, v in vals.items()}, grads, masks


def evaluate_warps(inp, dtype):
    """the per-view warps of PatchProjector in `dtype` -> pixel colours [N,S,V,3], mask [N,S,V], patch colours
    [N,S,V,Npx,3], mask [N,S,V,Npx]"""
    with default_dtype(dtype):
        intr, w2cs, c2ws, qc2w = cameras(inp, dtype)
        pts, imgs = inp["pts"].to(dtype), inp["imgs"].to(dtype)
        pcol, pmask = O.pixel_warp(pts, imgs, intr, w2cs)
        tcol, tmask = O.patch_warp(pts, inp["rays_uv"].to(dtype), inp["normals"].to(dtype), imgs, intr[0], intr, qc2w, c2ws,
                                   inp["hps"])
    return pcol, pmask.bool(), tcol, tmask.bool()


# ------------------------------------------------------------------------------------------------------------------ #
# the decisions and their margins
# ------------------------------------------------------------------------------------------------------------------ #
def geometry(inp, dtype=torch.float64, normals=None):
    """every quantity a kernel of csrc/blend.hip thresholds, in `dtype`, with the decision taken on it.
    xn, yn [N,S,V] (pixel_blend / pixel_warp: in bounds = |xn| < 1 and |yn| < 1); pn [N,S] (inside = |p| < 1);
    cs [N,S] (normal flip: its sign); d1 [N,S], d2 [N,S,V] (homography valid = |d1| > 1e-3, |d1 - d2| > 1e-3,
    d2 / d1 < 1); t2, gx, gy [N,S,V,Npx] (patch pixel valid = t2 > 0, h <= gx < W - h, h <= gy < H - h)."""
    intr, w2cs, c2ws, qc2w = cameras(inp, dtype)
    pts = inp["pts"].to(dtype)
    H, W, hps = inp["H"], inp["W"], inp["hps"]
    proj = torch.matmul(intr[:, :3, :3], w2cs[:, :3, :])
    pc = torch.einsum("vij,nsj->nsvi", proj[:, :, :3], pts) + proj[:, :, 3]
    zc = pc[..., 2].clamp(min=1e-3)
    xn = 2 * (pc[..., 0] / zc) / (W - 1) - 1
    yn = 2 * (pc[..., 1] / zc) / (H - 1) - 1
    out = dict(W=W, xn=xn, yn=yn, pix_mask=(xn.abs() < 1) & (yn.abs() < 1),
               pn=torch.linalg.norm(pts, dim=-1))
    out["inside"] = out["pn"] < 1.0
    if hps is None:
        return out
    if normals is None:
        grad, rd = inp["grad"].to(dtype), inp["rays_d"].to(dtype)
        gn = grad / (torch.linalg.norm(grad, dim=-1, keepdim=True) + 1e-5)
        cs = (rd[:, None] * gn).sum(-1)
        nrm = torch.where(cs > 0, -1.0, 1.0).to(dtype)[..., None] * gn
    else:
        cs, nrm = None, normals.to(dtype)
    Kri, Ks = torch.inverse(intr[0, :3, :3]), intr[:, :3, :3]
    inv_ref = torch.inverse(qc2w)
    rel = torch.inverse(c2ws) @ qc2w
    Rr, tr, Rl, tl = inv_ref[:3, :3], inv_ref[:3, 3], rel[:, :3, :3], rel[:, :3, 3]
    c2 = -(Rl.transpose(1, 2) @ tl[..., None])[..., 0]                       # [V,3]
    rn = nrm @ Rr.t()
    pr = pts @ Rr.t() + tr
    d1 = (rn * pr).sum(-1)                                                   # [N,S]
    d2 = rn @ c2.t()                                                         # [N,S,V]
    valid = (d1.abs()[..., None] > 1e-3) & ((d1[..., None] - d2).abs() > 1e-3) & ((d2 / d1[..., None]) < 1)
    sg = torch.where(d1 < 0, -1.0, 1.0).to(dtype)
    dd = d1.abs().clamp(min=1e-8) * sg
    sdist = torch.linalg.norm(pts - qc2w[:3, 3], dim=-1)
    zax = torch.zeros(3, dtype=dtype)
    zax[2] = 1.0
    q = torch.where(valid[..., None], (rn / dd[..., None])[:, :, None, :], (zax / sdist[..., None])[:, :, None, :])
    M1 = Rl[None, None] + tl[None, None, :, :, None] * q[..., None, :]       # [N,S,V,3,3]
    Hm = Ks[None, None] @ M1 @ Kri
    uv = torch.stack([(inp["rays_uv"][:, 0].to(dtype) + 1) / 2. * (W - 1), (inp["rays_uv"][:, 1].to(dtype) + 1) / 2. * (H - 1)],
                     -1)
    px = uv[:, None, :] + O.patch_offsets(hps).to(dtype)
    hom = torch.cat([px, torch.ones(px.shape[0], px.shape[1], 1, dtype=dtype)], -1)
    t = torch.einsum("nsvij,npj->nsvpi", Hm, hom)
    t2 = t[..., 2]
    den = t2.clamp(min=1e-8)
    gx, gy = t[..., 0] / den, t[..., 1] / den
    out.update(cs=cs, d1=d1, d2=d2, valid_h=valid, t2=t2, gx=gx, gy=gy,
               patch_mask=(t2 > 0) & (gx < W - hps) & (gy < H - hps) & (gx >= hps) & (gy >= hps))
    return out


def pixel_margin(geo, geo32):
    """[N,S,V,1] the margin on source-image coordinates of each (sample, view): PIX_MARGIN, or MOVE_FACTOR x what fp32
    moves that homography's in-front pixels where that is more.  The plane term t n^T / d1 of a homography makes its
    coordinates ill-conditioned as 1 / d1^2 (d1 = n . p carries ~5e-7 of absolute rounding error, the term is ~f |t| / d1
    pixels), so no single constant covers d1 ~ 0.1; the fp32 evaluation of the same expression measures it."""
    W = geo["W"]            # pixels further than an image width away are outside whatever fp32 does to them
    front = (geo["t2"] > 1e-3) & (geo["gx"].abs() < 2 * W) & (geo["gy"].abs() < 2 * W)
    mv = torch.maximum((geo32["gx"].double() - geo["gx"]).abs(), (geo32["gy"].double() - geo["gy"]).abs())
    mv = torch.where(front, mv, torch.zeros_like(mv)).max(dim=-1, keepdim=True)[0]
    return (MOVE_FACTOR * mv).clamp(min=PIX_MARGIN)


def ties(inp, geo=None, normals=None, margin=MARGIN, geo32=None):
    """which decisions of `geometry` (float64) are within the margins.  -> dict of bool tensors:
    pix [N,S,V], inside [N,S], flip [N,S], homography [N,S,V], patch_pixel [N,S,V,Npx] (the pixel's own mask),
    view [N,S,V] (the view's usability at the sample: not robust unless some pixel is outside by more than the margin or
    all are inside by more than it, or its homography is tied)."""
    geo = geometry(inp, torch.float64, normals) if geo is None else geo
    H, W, hps = inp["H"], inp["W"], inp["hps"]
    if hps is not None:
        pix_margin = pixel_margin(geo, geometry(inp, torch.float32, normals) if geo32 is None else geo32)
    # in bounds <=> min(1 - |xn|, 1 - |yn|) > 0
    out = dict(pix=torch.minimum(1 - geo["xn"].abs(), 1 - geo["yn"].abs()).abs() < margin,
               inside=(geo["pn"] - 1.0).abs() < margin)
    if hps is None:
        return out
    d1, d2 = geo["d1"][..., None], geo["d2"]
    out["flip"] = (geo["cs"].abs() < margin) if geo["cs"] is not None else torch.zeros_like(out["inside"])
    out["homography"] = ((d1.abs() - 1e-3).abs() < margin) | (((d1 - d2).abs() - 1e-3).abs() < margin) | \
                        ((d2 / d1 - 1).abs() < margin)
    # signed distances inside, each in units of its margin: the pixel is valid <=> all > 0
    gx, gy = geo["gx"], geo["gy"]
    sd = torch.stack([geo["t2"] / margin, (W - hps - gx) / pix_margin, (H - hps - gy) / pix_margin, (gx - hps) / pix_margin,
                      (gy - hps) / pix_margin]).min(dim=0)[0]
    rob_in, rob_out = sd > 1, sd < -1
    out["patch_pixel"] = ~(rob_in | rob_out) | out["homography"][..., None]
    out["view"] = ~(rob_out.any(-1) | rob_in.all(-1)) | out["homography"]
    return out


def kept_rays(inp, t):
    """rays none of whose decisions is tied (t = ties(inp)): the rows compared -- the patch outputs, the colour and every
    gradient of a ray depend on all decisions of all its samples"""
    bad = t["pix"].any(-1).any(-1)
    if inp.get("bg_in") is not None:
        bad = bad | t["inside"].any(-1)
    if inp["hps"] is not None:
        bad = bad | t["flip"].any(-1) | t["view"].any(-1).any(-1)
    return ~bad


@functools.lru_cache(maxsize=None)
def reference(idx):
    """inp (the inputs of the reference's rays), rows (their numbers in the full case), geo / geo32 (geometry in float64 /
    fp32), ties, keep (rays compared), v64 / g64 / m64 and v32 / g32 / m32 (values, gradients, masks of `evaluate`) of
    CASES[idx]; computed once and shared -- callers leave the tensors unchanged"""
    full = make_case(idx)
    rows = ref_rays(full["N"])
    inp = take_rays(full, rows)
    geo, geo32 = geometry(inp), geometry(inp, torch.float32)
    t = ties(inp, geo, geo32=geo32)
    v64, g64, m64 = evaluate(inp, torch.float64)
    v32, g32, m32 = evaluate(inp, torch.float32)
    return dict(inp=inp, rows=rows, geo=geo, geo32=geo32, ties=t, keep=kept_rays(inp, t), v64=v64, g64=g64, m64=m64, v32=v32,
                g32=g32, m32=m32)


@functools.lru_cache(maxsize=None)
def warp_reference(idx):
    """inp, geo / geo32, ties, w64 / w32 (`evaluate_warps` in float64 / fp32) of WARP_CASES[idx]"""
    inp = make_warp_case(idx)
    geo, geo32 = geometry(inp, torch.float64, inp["normals"]), geometry(inp, torch.float32, inp["normals"])
    return dict(inp=inp, geo=geo, geo32=geo32, ties=ties(inp, geo, geo32=geo32), w64=evaluate_warps(inp, torch.float64),
                w32=evaluate_warps(inp, torch.float32))


def conditions(idx):
    """what the generator promises about CASES[idx], measured on the float64 reference -> dict"""
    c, r = CASES[idx], reference(idx)
    inp, m64 = r["inp"], r["m64"]
    out = dict(no_pixel_view=int((~m64["pix"].any(-1)).sum()), samples=inp["N"] * inp["S"],
               inside_share=float(m64["inside"].float().mean()), tie_share=1.0 - float(r["keep"].float().mean()))
    if c["hps"] is not None:
        usable = m64["patch"].all(-1)                                       # [N,S,V]
        out.update(usable_share=float(usable.float().mean()), no_patch_view=int((~usable.any(-1)).sum()),
                   pixel_tie_share=float(r["ties"]["patch_pixel"].float().mean()))
        if npx_of(c["hps"]) > 64:
            out["second_chunk_decides"] = int((m64["patch"][..., :64].all(-1) & ~m64["patch"][..., 64:].all(-1)).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# the launch under test (the one function here that needs the GPU)
# ------------------------------------------------------------------------------------------------------------------ #
def launch(dev, inp, hwc=False):
    """blend_and_composite forward + backward of sum(color_pixel k1) + sum(patch_colors k2) on the fp32 inputs of a case
    -> (values, gradients) on the host, named as `evaluate` names them, plus d_w_patch: the patch launch's own d w
    [N,S+n_out].  hwc: the source images as an NCHW view of channel-interleaved memory."""
    from neuraludf_amd.models import blend
    D = lambda t: None if t is None else t.to(dev)
    L = lambda t: None if t is None else t.detach().clone().to(dev).requires_grad_(True)
    lg, w, bg_in, bg_tail = L(inp["logits"]), L(inp["w"]), L(inp["bg_in"]), L(inp["bg_tail"])
    imgs = D(inp["imgs"])
    if hwc:
        imgs = imgs.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not imgs.is_contiguous()
    uv = D(inp["rays_uv"].clone()) if inp["hps"] is not None else None
    cp, pc, pm = blend.blend_and_composite(inp["hps"], D(inp["pts"]), lg, w, D(inp.get("grad")), D(inp["rays_d"]), imgs,
                                           D(inp["w2cs"]), D(inp["intrinsics"]), D(inp["query_c2w"]), uv, bg_in=bg_in,
                                           bg_tail=bg_tail)
    vals, grads = dict(color_pixel=cp), {}
    f = (cp * D(inp["k1"])).sum()
    if pc is not None:
        vals.update(patch_colors=pc, patch_mask=pm)
        fp = (pc * D(inp["k2"])).sum()
        grads["d_w_patch"] = torch.autograd.grad(fp, w, retain_graph=True)[0]
        f = f + fp
    f.backward()
    G = lambda t: None if t is None else t.grad
    grads.update(d_logits=G(lg), d_w=G(w), d_bg_in=G(bg_in), d_bg_tail=G(bg_tail))
    C = lambda d: {k: None if v is None else v.detach().cpu() for k, v in d.items()}
    return C(vals), C(grads)


# ------------------------------------------------------------------------------------------------------------------ #
# error measure and bound
# ------------------------------------------------------------------------------------------------------------------ #
def floor_of(name):
    return GRAD_FLOOR if name.startswith("d_") else VALUE_FLOOR


def error(a, b, keep=None):
    """max |a - b| / max |b| over the rows kept (b = float64)"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    if keep is not None:
        a, b = a[keep], b[keep]
    return tensor_error(a, b)


def bound(name, e_ref):
    """min(max(FACTOR e_ref, floor), CAP) with composite_ref's numbers: e_ref = the fp32 oracle's own distance from float64
    on the same case, tensor and rows"""
    return min(max(FACTOR * e_ref, floor_of(name)), CAP)


def hold(case, r, vals, grads, rows_out, fails):
    """the bound for every output of a launch on the full case against the reference of `r["rows"]`, over the rays kept.
    Prints each figure; appends (case, tensor, err, e_ref, bound, max|ref|) to rows_out and misses to fails."""
    rows, keep = r["rows"], r["keep"]
    for got, r64, r32, names in ((vals, r["v64"], r["v32"], VALUES), (grads, r["g64"], r["g32"], GRADS)):
        for nm in names:
            if r64.get(nm) is None:
                continue
            e, er = error(got[nm][rows], r64[nm], keep), error(r32[nm], r64[nm], keep)
            bd = bound(nm, er)
            print("%s %-12s err %.2e e_ref %.2e bound %.1e err/e_ref %.2f" % (case, nm, e, er, bd, e / max(er, 1e-300)))
            rows_out.append((case, nm, e, er, bd, float(r64[nm][keep].abs().max())))
            if not e <= bd:
                fails.append("%s %s: err %.3e > bound %.1e (e_ref %.2e)" % (case, nm, e, bd, er))
