"""No live result may depend on memory nobody wrote.

Every buffer of the hot path is a torch.empty, and the chain kernels' buffers carry pad_rows(P) rows of which only P are live
(include/nudf.h: scratch rows may hold any bit pattern on entry; no live output, maximum or status bit may depend on them).  On
a fresh allocation the scratch holds zeros or the finite leftovers of the previous test, so a leak shows only when the memory
is poisoned on purpose: tests/scratch_poison.py fills every floating-point torch.empty with NaN, +Inf, -1e30 or 1e5, and every
run here must give the SAME BITS as the run whose allocations were filled with 0.0 -- gradients repeat bit for bit between two
runs (test_gpu_arch_sweep.py), so the property is exact and has no tolerance.  The clean leg is held to the float64 bars of
tests/arch_cases.py, which keeps "identical" from meaning "identically wrong".  The status word stays 0 throughout.

  * engine level: the networks of tests/arch_cases.py off the shipped shapes, one forward + input gradient + backward of the
    random-weighted sum of all outputs, at P = 1, 33, 97 (ragged against the 32-point tile) and 349 (tile forced to 64) -- all
    with P % 4 == 1, for the 4-point packed quads -- in five arithmetic modes, with the two UDF sweeps fused and unfused, and
    once per entry on the per-layer path;
  * one whole render with gradients (37 rays x 27 + 8 samples: the point counts are ragged against 64, 32 and 4), the same
    render through its blending branch (3 source views, rays_uv, 7 x 7 patches) and the 5-ray minimum-sample case of
    test_gpu_edges.py;
  * the colour-loss, step-loss and blend-loss autograd functions at 37 rays, with and without a mask;
  * three eager train steps at the same ragged batch, without and with the blending branch (pixel and patch colour terms).
The blend kernels alone, ray batching and the mesh tools: tests/test_gpu_blend_poison.py, tests/test_gpu_mesh_poison.py.

If a combination is not bit-repeatable even clean against clean, the test says so on stdout and holds each poisoned leg to one
of two clean runs instead.

What failed on the kernels before this test existed (one run of the previous library, each a failed assertion; DESIGN.md
section 4.1l has the table): test_engine_results_do_not_depend_on_unwritten_memory for the four UDF entries in the three bf16x3
modes, in every unfused combination -- the element-wise INIT_SEED stored DA[L-1] for live rows only, and the scratch rows
reached the adjoint sweep's maxima and the scale of the f16x2 weight-gradient GEMM: finite wrong weight gradients under -1e30
and 1e5 at every P, under +Inf at P = 1, never under NaN, status word 0.  Everything else passed there."""
import functools
import math

import pytest
import torch

import arch_cases as A
import scratch_poison as SP
import test_gpu_arch_sweep as S
from common import build_modules, grel, perturb_
from oracle import udf_oracle as O

pytestmark = pytest.mark.gpu

POINTS = ((1, 0), (33, 0), (97, 0), (349, 64))       # (P, forced tile)
ENTRIES = ("u100", "u250", "u64nw", "c100", "n64", "u_f100+c_f100")
MODES = {
    "fp32": dict(precision="fp32"),
    "bf16x3": dict(precision="bf16x3"),                                             # the default: f16x2 sweeps
    "bf16x3-six": dict(precision="bf16x3", fwd_split="0", bwd_f16x2=False),         # six bf16 products everywhere
    "mixed16": dict(precision="mixed16"),
    "bf16x3-exstored": dict(precision="bf16x3", ex_fly=False),                      # the tangent sweep stores EX
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class _mode:
    """every module-level switch of mlp that selects a kernel or a buffer, for one block, restored whatever happens"""

    def __init__(self, precision="bf16x3", fwd_split=None, bwd_f16x2=None, ex_fly=None, tile=0, use_chain=True, fuse=True):
        self.kw = dict(precision=precision, fwd_split=fwd_split, bwd_f16x2=bwd_f16x2, ex_fly=ex_fly, tile=tile,
                       use_chain=use_chain, fuse=fuse)

    def __enter__(self):
        from neuraludf_amd import mlp
        k = self.kw
        self.old = (mlp.PRECISION, mlp.FWD_F16X2, mlp.BWD_F16X2, mlp.EX_FLY, mlp.CHAIN_TILE, mlp.USE_CHAIN, mlp.FUSE_SWEEPS)
        mlp.set_precision(k["precision"])
        if k["fwd_split"] is not None:
            mlp.set_fwd_split(k["fwd_split"])
        if k["bwd_f16x2"] is not None:
            mlp.BWD_F16X2 = k["bwd_f16x2"]
        if k["ex_fly"] is not None:
            mlp.EX_FLY = k["ex_fly"]
        mlp.CHAIN_TILE, mlp.USE_CHAIN = k["tile"], k["use_chain"]
        mlp.set_fuse_sweeps(k["fuse"])

    def __exit__(self, *exc):
        from neuraludf_amd import mlp
        (mlp.PRECISION, mlp.FWD_F16X2, mlp.BWD_F16X2, mlp.EX_FLY, mlp.CHAIN_TILE, mlp.USE_CHAIN, mlp.FUSE_SWEEPS) = self.old
        return False


def _status(dev, clear=False):
    from neuraludf_amd import _lib
    return _lib.read_status(dev, clear=clear)


def _same(a, b):
    """names of the tensors of two {name: tensor} results that are not bit-equal"""
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    return [k for k in a if not (a[k].shape == b[k].shape and torch.equal(a[k], b[k]))]


def _legs(run, dev, engines, tag, differ=_same, equal=torch.equal):
    """the clean leg twice and one leg per poison -> (clean result, [failure strings]).  `run()` -> {name: tensor}.
    differ(a, b) names the tensors of two results that differ and equal(x, y) compares two tensors: _same / torch.equal here,
    the bit comparison of scratch_poison.same_bits where a result may legitimately hold NaN."""
    res = {}
    _status(dev, clear=True)
    bits = {}
    for v in (SP.CLEAN, SP.CLEAN) + SP.POISONS:
        with SP.poisoned(v, engines=engines):
            r = run()
            torch.cuda.synchronize()
        key = SP.label(v) if SP.label(v) not in res else SP.label(v) + " (again)"
        res[key] = r
        bits[key] = _status(dev, clear=True)
    clean, again = res[SP.label(SP.CLEAN)], res[SP.label(SP.CLEAN) + " (again)"]
    bad = []
    unstable = differ(clean, again)
    if unstable:
        print(f"scratch poison [{tag}]: NOT bit-repeatable clean against clean: {unstable}")
    for v in SP.POISONS:
        r = res[SP.label(v)]
        d = differ(r, clean)
        if d and unstable:
            d = [k for k in d if not equal(r[k], again[k])]
        if d:
            bad.append(f"{tag} poison {SP.label(v)}: differs from the clean leg in {d}")
    for k, b in bits.items():
        if b:
            bad.append(f"{tag} leg {k}: status word {b}")
    return clean, bad


# ---------------------------------------------------------------------------------------------------------------------
# 1. engine level
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_reference(P):
    """float64 oracle of UDF network -> colour network (F = 100) in the renderer's layout, and the float32 oracle's distance
    from it (as test_gpu_arch_sweep.test_colour_adjoint_enters_the_udf_adjoint_load forms it)"""
    iu, ic = A.inputs(A.ALL["u_f100"], P), A.inputs(A.ALL["c_f100"], P)
    x, dirs, w, wg = iu["x"], ic["dirs"], ic["w"], iu["wg"]

    def oracle(dtype):
        c = lambda t: t.detach().to(dtype).clone()
        su, sc = A.oracle_sd(A.module("u_f100")[1], dtype), A.oracle_sd(A.module("c_f100")[1], dtype)
        y = O.udf_forward(su, c(x), A.ALL["u_f100"]["cfg"])
        g = O.udf_gradient(su, c(x), A.ALL["u_f100"]["cfg"], create_graph=True)
        out = O.color_forward(sc, c(x), None, c(dirs), y[:, 1:], A.ALL["c_f100"]["cfg"])
        (sum((a * c(b)).sum() for a, b in zip(out, w)) + (g * c(wg)).sum()).backward()
        grads = {"udf." + n: t.grad.detach() for n, t in su.items()}
        grads.update({"color." + n: t.grad.detach() for n, t in sc.items()})
        vals = dict(color_base=out[0].detach(), color=out[1].detach(), logits=out[2].detach(), grad=g.detach())
        return vals, grads

    v64, g64 = oracle(torch.float64)
    v32, g32 = oracle(torch.float32)
    return dict(inp=dict(x=x, dirs=dirs, w=w, wg=wg), vals=v64, grads=g64, e_vals={k: A.rel(v32[k], v64[k]) for k in v64},
                e_grads={k: grel(g32[k], g64[k]) for k in g64})


def _run_pair(inp, dev):
    udf, col = S._net("u_f100", dev), S._net("c_f100", dev)
    ceng = col.engine()
    D = lambda t: t.to(dev)
    udf.zero_grad()
    col.zero_grad()
    _, CIN, g = udf.evaluate(D(inp["x"]), want_grad=True, feat_ld=ceng.cin_ld)
    out = col.evaluate(CIN, D(inp["dirs"]), 1)
    (sum((a * D(b)).sum() for a, b in zip(out, inp["w"])) + (g * D(inp["wg"])).sum()).backward()
    torch.cuda.synchronize()
    vals = dict(color_base=out[0], color=out[1], logits=out[2], grad=g)
    grads = {"udf." + n: p.grad.detach().clone() for n, p in udf.named_parameters()}
    grads.update({"color." + n: p.grad.detach().clone() for n, p in col.named_parameters()})
    return {k: v.detach().clone() for k, v in vals.items()}, grads


def _engine_case(entry, P, dev):
    """-> (run() -> (values, gradients), engines, reference)"""
    if "+" in entry:
        ref = _pair_reference(P)
        engines = [S._net("u_f100", dev).engine(), S._net("c_f100", dev).engine()]
        return (lambda: _run_pair(ref["inp"], dev)), engines, ref
    ref = A.reference(entry, P)
    return (lambda: S._run(entry, ref["inp"], dev)), [S._net(entry, dev).engine()], ref


def _flat(run):
    """values (live rows: the engines return [:P] views) and gradients as one {name: tensor}"""
    vals, grads = run()
    out = {"value " + k: v for k, v in vals.items()}
    out.update({"gradient " + k: v for k, v in grads.items()})
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_engine_results_do_not_depend_on_unwritten_memory(dev, entry, mode):
    """values on live rows, every parameter gradient and d_feat: torch.equal to the clean leg under each poison; the clean leg
    within the float64 bars of arch_cases (not mixed16, which has no such bar)"""
    combos = [(P, tile, True, fuse) for P, tile in POINTS for fuse in (True, False)]
    if mode == "bf16x3":
        combos.append((97, 0, False, True))              # the per-layer path, once per entry
    bad = []
    for P, tile, use_chain, fuse in combos:
        run, engines, ref = _engine_case(entry, P, dev)
        tag = f"{entry} {mode} P={P} tile={tile or 'auto'} {'chain' if use_chain else 'layers'} {'fused' if fuse else 'unfused'}"
        with _mode(tile=tile, use_chain=use_chain, fuse=fuse, **MODES[mode]):
            clean, b = _legs(lambda: _flat(run), dev, engines, tag)
        bad += b
        if mode != "mixed16" and fuse:                    # once per (entry, P, mode): the float64 bars of arch_cases
            vals = {k[6:]: v for k, v in clean.items() if k.startswith("value ")}
            grads = {k[9:]: v for k, v in clean.items() if k.startswith("gradient ")}
            S._against_float64(tag, vals, grads, ref)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. render, losses, train step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(dev):
    from neuraludf_amd.models import fields
    mods = perturb_(build_modules(fields, seed=0))
    for m in mods.values():
        m.to(dev)
    return mods


RENDERS = {
    # 37 rays: N % 4 == 1; 37 x 27 = 999 core points and 37 x 17 = 629 coarse points, ragged against 64, 32 and 4
    "ragged": (37, dict(n_samples=17, n_importance=10, n_outside=8, up_sample_steps=2, perturb=0.0)),
    # the minimum sample counts of test_gpu_edges.py
    "minimum": (5, dict(n_samples=2, n_importance=3, n_outside=0, up_sample_steps=3, perturb=0.0)),
    # the ragged case through the blending branch: 3 source views (channel-interleaved, as the dataset hands them over) and
    # rays_uv, so that pixel_blend, pixel_composite and patch_blend (7 x 7 patches) run forward and backward
    "ragged_blend": (37, dict(n_samples=17, n_importance=10, n_outside=8, up_sample_steps=2, perturb=0.0, h_patch_size=3)),
}


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", list(RENDERS))
def test_render_and_its_backward_do_not_depend_on_unwritten_memory(dev, nets, case, fuse):
    """every entry of the output dict and every parameter gradient of a fixed weighted sum of the differentiable outputs; with
    the UDF value and input-gradient sweeps as one launch (the default) and as two"""
    from neuraludf_amd import synth
    from neuraludf_amd.models.udf_renderer_blending import UDFRendererBlending
    n_rays, kw = RENDERS[case]
    rend = UDFRendererBlending(nets["nerf"], nets["udf"], nets["var"], nets["color"], nets["beta"], **kw)
    r = synth.make_rays(synth.make_scene("tiny"), 0, n_rays, seed=1900 + n_rays)
    r = {k: v[:n_rays].to(dev) for k, v in r.items()}
    gen = torch.Generator().manual_seed(n_rays)
    weights = {}
    src = None
    if case.endswith("_blend"):
        src = {k: v.to(dev) for k, v in synth.make_source_views(synth.make_scene("tiny"), 0, 3, hwc=True).items()}

    def run():
        for m in nets.values():
            m.zero_grad()
        kw_blend = {}
        if src is not None:          # (the patch launch rescales rays_uv in place: a fresh copy per run)
            kw_blend = dict(color_maps=src["color_maps"], w2cs=src["w2cs"], intrinsics=src["intrinsics"],
                            query_c2w=src["query_c2w"], rays_uv=r["rays_uv"].clone())
        out = rend.render(r["rays_o"], r["rays_d"], r["near"], r["far"], cos_anneal_ratio=0.5, flip_saturation=0.5,
                          perturb_overwrite=0, **kw_blend)
        loss = 0.0
        for k in sorted(out):
            v = out[k]
            if torch.is_tensor(v) and v.is_floating_point() and v.requires_grad:
                if k not in weights:        # fixed weights, drawn once on the host
                    weights[k] = torch.randn(v.shape, generator=gen).to(dev)
                loss = loss + (v * weights[k]).sum()
        loss.backward()
        torch.cuda.synchronize()
        res = {"out " + k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
        for name, m in nets.items():
            for pn, p in m.named_parameters():
                if p.grad is not None:
                    res[f"gradient {name}.{pn}"] = p.grad.detach().clone()
        return res

    engines = [m.engine() for m in nets.values() if hasattr(m, "engine")]
    with _mode(fuse=fuse):
        clean, bad = _legs(run, dev, engines, f"render {case} {'fused' if fuse else 'unfused'}")
    assert len([k for k in clean if k.startswith("gradient ")]) > 50 and "out color" in clean and "out z_vals" in clean
    if src is not None:
        assert {"out color_pixel", "out patch_colors", "out patch_mask"} <= set(clean)
        assert clean["out patch_colors"].shape == (n_rays, 49, 3) and float(clean["out color_pixel"].abs().max()) > 0
    assert all(bool(torch.isfinite(v.float()).all()) for v in clean.values()), [k for k, v in clean.items()
                                                                                  if not bool(torch.isfinite(v.float()).all())]
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def loss_setup(dev):
    from neuraludf_amd.train import Trainer
    rconf = dict(n_samples=32, n_importance=16, n_outside=0, up_sample_steps=2, perturb=1.0, upsampling_type="mix",
                 use_norm_grad_for_cosine=True, h_patch_size=3)
    tr = Trainer(dev, rconf, color_loss_conf=dict(color_pixel_weight=0.5, color_patch_weight=0.1), seed=0,
                 train_conf=dict(igr_ns_weight=0.05, sparse_weight=0.01))
    return tr.color_loss, tr.loss_weights().device(dev)


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("which", ["colour", "step", "blend"])
def test_loss_functions_do_not_depend_on_unwritten_memory(dev, loss_setup, which, masked):
    """forward values and every input gradient (the d_* buffers are empty_like: the kernels must write all of them)"""
    from neuraludf_amd.loss.loss import _ColorLossFn, _StepLossFn
    closs, w_dev = loss_setup
    n = 37
    g = torch.Generator().manual_seed(37 + masked)
    R = lambda *s: torch.rand(*s, generator=g).to(dev)
    cb0, c0, pix0, gt = R(n, 3), R(n, 3), R(n, 3), R(n, 3)
    pc0, gp = R(n, 49, 3), R(n, 49, 3)
    sums0 = (R(5) + 0.5) * n
    wsum = R(n, 1)
    mask = (torch.rand(n, 1, generator=g) > 0.3).float().to(dev)
    pm = (torch.rand(n, generator=g) > 0.3).to(dev) if masked else torch.ones(n, dtype=torch.bool, device=dev)

    def run():
        leaf = lambda t: t.detach().clone().requires_grad_(True)
        cb, c, pix, pc, sums = leaf(cb0), leaf(c0), leaf(pix0), leaf(pc0), leaf(sums0)
        if which == "colour":
            out = _ColorLossFn.apply(cb, c, gt, mask if masked else None, w_dev, False)
            (out[0] + 0.5 * out[1] + 0.25 * out[2]).backward()
            ins = dict(cb=cb, c=c)
        elif which == "step":
            out = _StepLossFn.apply(cb, c, gt, mask if masked else None, sums, float(n), w_dev)
            out[0].backward()
            ins = dict(cb=cb, c=c, sums=sums)
        else:
            out = closs.blend_step_loss(cb, c, gt, pix, pc, gp, pm, wsum, sums, float(n), w_dev)
            out[0].backward()
            ins = dict(cb=cb, c=c, pix=pix, pc=pc, sums=sums)
        torch.cuda.synchronize()
        res = {f"out {i}": o.detach().clone() for i, o in enumerate(out)}
        for k, t in ins.items():
            assert t.grad is not None, k
            res["d " + k] = t.grad.detach().clone()
        return res

    clean, bad = _legs(run, dev, (), f"{which} loss n={n} {'mask' if masked else 'no mask'}")
    assert all(bool(torch.isfinite(v.float()).all()) for v in clean.values())
    assert any(float(v.abs().max()) > 0 for k, v in clean.items() if k.startswith("d "))
    assert not bad, "\n".join(bad)


def _train_steps(dev, rconf, loss_conf, with_views):
    """three eager steps (render, loss, backward, Adam) at a ragged batch: losses and every parameter after step 3, clean
    against the poisons -1e30 and NaN"""
    from neuraludf_amd import synth
    from neuraludf_amd.train import Trainer
    scene = synth.make_scene("tiny")
    batches = [{k: v.to(dev) for k, v in synth.make_rays(scene, i % 3, 37, seed=60 + i).items()} for i in range(3)]
    blends = [None] * 3
    if with_views:
        g = torch.Generator().manual_seed(61)
        for i, batch in enumerate(batches):
            batch["gt_patch_colors"] = torch.rand(37, 49, 3, generator=g).to(dev)
            blends[i] = {k: v.to(dev) for k, v in synth.make_source_views(scene, i % 3, 3, hwc=True).items()}

    def run(value):
        _status(dev, clear=True)
        with SP.poisoned(value):
            tr = Trainer(dev, rconf, color_loss_conf=loss_conf, seed=0, fused_adam=True)
            torch.manual_seed(77)
            losses = []
            for i, batch in enumerate(batches):
                loss, out = tr.step(batch, cos_anneal_ratio=0.5 + 0.1 * i, flip_saturation=0.3 * i, perturb_overwrite=0,
                                    blend=blends[i])
                assert (out.get("patch_colors") is not None) == with_views
                losses.append(loss.detach().clone())
            torch.cuda.synchronize()
            res = {f"loss {i}": l for i, l in enumerate(losses)}
            k = 0
            for grp in tr.param_groups:
                for p in grp:
                    res[f"parameter {k}"] = p.detach().clone()
                    k += 1
        return res, _status(dev, clear=True)

    clean, bits = run(SP.CLEAN)
    assert bits == 0 and all(bool(torch.isfinite(v).all()) for v in clean.values())
    bad = []
    for v in (-1e30, math.nan):
        r, b = run(v)
        d = _same(r, clean)
        if d:
            bad.append(f"train steps, poison {SP.label(v)}: differs from the clean leg in {d}")
        if b:
            bad.append(f"train steps, poison {SP.label(v)}: status word {b}")
    assert not bad, "\n".join(bad)


def test_train_steps_do_not_depend_on_unwritten_memory(dev):
    """three eager steps (render, loss, backward, Adam) at a ragged batch: losses and every parameter after step 3.  No graph
    capture: a captured fill would change what is replayed."""
    _train_steps(dev, dict(n_samples=17, n_importance=10, n_outside=8, up_sample_steps=2, perturb=1.0), None, False)


def test_train_steps_with_blending_do_not_depend_on_unwritten_memory(dev):
    """the same three steps through the blending branch: 7 x 7 patches, pixel and patch colour terms in the loss, batches
    with 3 source views and ground-truth patches.  Eager only, for the same reason."""
    _train_steps(dev, dict(n_samples=17, n_importance=10, n_outside=8, up_sample_steps=2, perturb=1.0, h_patch_size=3),
                 dict(color_pixel_weight=0.5, color_patch_weight=0.1), True)
