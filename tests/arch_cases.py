"""Network shapes off the shipped conf's, for tests/test_gpu_arch_sweep.py: per entry the constructor kwargs of the module,
the matching oracle cfg and whether the engine's `_chain_ok()` gate must send it to the fused chain kernel.

Modules are built as common.build_modules does (seeded, the constructors' prints swallowed; that function builds the shipped
conf only) and perturbed BY common.perturb_ (the geometric initialisation zeroes the encoding columns, which would hide channel-order bugs).  The float64 / float32
oracle evaluations of an entry are computed once per (entry, point count) and shared by every test that needs them."""
import collections
import contextlib
import functools
import io

import torch

from common import grel, perturb_  # noqa: F401  (grel: the project's bound on gradients, used by the sweep through this module)
from oracle import udf_oracle as O

_UDF_BASE = dict(d_in=3, bias=0.5, scale=1.0, geometric_init=True, weight_norm=True, udf_type="abs")


def _udf(d_hidden, n_layers, skip_in, multires, d_out, chain=True, **kw):
    k = dict(_UDF_BASE, d_hidden=d_hidden, n_layers=n_layers, skip_in=tuple(skip_in), multires=multires, d_out=d_out, **kw)
    cfg = O.UDFCfg(d_in=3, d_out=d_out, d_hidden=d_hidden, n_layers=n_layers, skip_in=tuple(skip_in), multires=multires,
                   scale=1.0, udf_type=k["udf_type"])
    return dict(kind="udf", kw=k, cfg=cfg, chain=chain)


def _color(d_feature, mode, d_in, d_hidden, n_layers, multires_view, views, chain=True):
    k = dict(d_feature=d_feature, mode=mode, d_in=d_in, d_out=3, d_hidden=d_hidden, n_layers=n_layers, weight_norm=True,
             multires_view=multires_view, squeeze_out=True, blending_cand_views=views)
    cfg = O.ColorCfg(d_feature=d_feature, mode=mode, d_in=d_in, d_out=3, d_hidden=d_hidden, n_layers=n_layers,
                     multires_view=multires_view, blending_cand_views=views)
    return dict(kind="color", kw=k, cfg=cfg, chain=chain)


def _nerf(D, W, multires, multires_view, skips, chain=True):
    k = dict(D=D, d_in=4, d_in_view=3, W=W, multires=multires, multires_view=multires_view, output_ch=4, skips=list(skips),
             use_viewdirs=True)
    cfg = O.NerfCfg(D=D, W=W, d_in=4, d_in_view=3, multires=multires, multires_view=multires_view, skips=tuple(skips))
    return dict(kind="nerf", kw=k, cfg=cfg, chain=chain)


# Entries the gate must send to the chain kernel.  (layer widths: E = 3 (2 multires + 1) encoding columns; the layer in front
# of the skip is d_hidden - E wide, and the encoding joins the tile at that column)
CHAIN = {
    "u64": _udf(64, 4, (2,), 4, 65),           # tail at column 37, E = 27
    "u100": _udf(100, 5, (3,), 10, 34),        # width no multiple of 4 or 16, F = 33 odd, E = 63, tail at column 37
    "u96": _udf(96, 3, (), 6, 129),            # no skip, 3 column tiles
    "u250": _udf(250, 8, (4,), 15, 257),       # E = 93 (nudf_posenc_vjp takes 96), 157 wide in front of the skip
    # fewest layers with a skip, the 'square' head.  d_hidden = 32 leaves 32 - E columns in front of the skip, so the
    # encoding must be narrower than 32: multires 4 (E = 27, a 5-wide layer) -- with multires 6 (E = 39) the module cannot
    # be constructed at all
    "u32sq": _udf(32, 2, (1,), 4, 33, udf_type="square"),
    "u64nw": _udf(64, 4, (2,), 6, 65, weight_norm=False),      # g == NULL pack / unpack paths, E = 39, tail at column 25
    "c64": _color(64, "no_normal", 6, 64, 2, 4, 4),
    "c100": _color(128, "idr", 12, 100, 3, 2, 10),
    "c29h": _color(256, "no_normal", 6, 128, 4, 4, 29),        # view head 3 + 29 = 32 wide, the limit
    "n64": _nerf(4, 64, 10, 4, [1]),
    "n96": _nerf(3, 96, 4, 2, []),
    # a pair with F = 100 (a multiple of 4, not of 16): the colour net's d CIN enters the UDF adjoint sweep's 112-column load
    "u_f100": _udf(64, 4, (2,), 4, 101),
    "c_f100": _color(100, "no_normal", 6, 64, 2, 4, 4),
}

# One step outside a gate each: `_chain_ok()` is False and the per-layer path serves the network.
GATE = {
    "g_u288": _udf(288, 3, (), 6, 33, chain=False),                        # wider than the 256 columns of a step
    "g_c33": _color(33, "no_normal", 6, 64, 2, 4, 4, chain=False),         # F % 4 != 0
    "g_c256v6": _color(256, "no_normal", 6, 256, 4, 6, 10, chain=False),   # k8(256 + 39 + 3) > 288
    # d_hidden = 256 with PE(dir) of 27 columns: the base head's 32-column tile would end at column 315 of the 288
    # (nudf_mlp_chain refuses the launch; the gate used to let it through)
    "g_c29": _color(256, "no_normal", 6, 256, 4, 4, 29, chain=False),
    "g_n100": _nerf(4, 100, 10, 4, [1], chain=False),                      # W % 32 != 0
}

# Refused before any kernel is launched (value + gradient evaluation).
REFUSED = {
    "r_2skips": (_udf(64, 4, (1, 2), 2, 33, chain=False), NotImplementedError),
    "r_E99": (_udf(128, 3, (), 16, 33), "NudfError"),                      # E = 99 > 96
}

ALL = dict(CHAIN, **GATE)


def build(entry, seed=0):
    """-> (module on the CPU, detached copy of its state dict)"""
    from neuraludf_amd.models import fields
    cls = {"udf": fields.UDFNetwork, "color": fields.ResidualRenderingNetwork, "nerf": fields.NeRF}[entry["kind"]]
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = cls(**entry["kw"])
    # (perturb_ walks the nerf, udf and colour modules of a set: the two this entry is not are empty)
    perturb_(collections.defaultdict(torch.nn.Module, {entry["kind"]: net}))
    return net, {n: t.detach().clone() for n, t in net.state_dict().items()}


def oracle_sd(sd, dtype, requires_grad=True):
    out = {}
    for k, v in sd.items():
        t = v.detach().clone().to(dtype)
        if requires_grad:
            t.requires_grad_(True)
        out[k] = t
    return out


def inputs(entry, P, seed=11):
    """seeded inputs and loss weights of an entry (float32, CPU)"""
    g = torch.Generator().manual_seed(seed + P)
    nrm = lambda t: torch.nn.functional.normalize(t, dim=-1)
    if entry["kind"] == "udf":
        return dict(x=torch.randn(P, 3, generator=g) * 0.7, wy=torch.randn(P, entry["kw"]["d_out"], generator=g),
                    wg=torch.randn(P, 3, generator=g))
    if entry["kind"] == "color":
        kw = entry["kw"]
        return dict(pts=torch.randn(P, 3, generator=g) * 0.6, dirs=nrm(torch.randn(P, 3, generator=g)),
                    nrm=nrm(torch.randn(P, 3, generator=g)), feat=torch.randn(P, kw["d_feature"], generator=g) * 0.5,
                    w=[torch.randn(P, 3, generator=g), torch.randn(P, 3, generator=g),
                       torch.randn(P, kw["blending_cand_views"], generator=g)])
    p3 = nrm(torch.randn(P, 3, generator=g))
    return dict(pts4=torch.cat([p3, torch.rand(P, 1, generator=g)], -1), dirs=nrm(torch.randn(P, 3, generator=g)),
                w=[torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g)])


def oracle_run(entry, sd, inp, dtype):
    """the oracle in `dtype` on the entry's inputs: values, the input gradient where the network has one, and every
    parameter gradient of the random-weighted sum of all outputs -> (values dict, grads dict)"""
    c = lambda t: t.detach().to(dtype).clone()      # (never the cached input itself: a leaf is made of one below)
    osd = oracle_sd(sd, dtype)
    cfg = entry["cfg"]
    if entry["kind"] == "udf":
        x = c(inp["x"])
        y = O.udf_forward(osd, x, cfg)
        gr = O.udf_gradient(osd, x, cfg, create_graph=True)
        ((y * c(inp["wy"])).sum() + (gr * c(inp["wg"])).sum()).backward()
        vals = dict(udf=y[:, 0], feat=y[:, 1:], grad=gr)
        extra = {}
    elif entry["kind"] == "color":
        fr = c(inp["feat"]).requires_grad_(True)
        out = O.color_forward(osd, c(inp["pts"]), c(inp["nrm"]), c(inp["dirs"]), fr, cfg)
        sum((a * c(b)).sum() for a, b in zip(out, inp["w"])).backward()
        vals = dict(color_base=out[0], color=out[1], logits=out[2])
        extra = {"d_feat": fr.grad}
    else:
        s, rgb = O.nerf_forward(osd, c(inp["pts4"]), c(inp["dirs"]), cfg)
        ((s * c(inp["w"][0])).sum() + (rgb * c(inp["w"][1])).sum()).backward()
        vals = dict(sigma=s, rgb=rgb)
        extra = {}
    grads = {n: t.grad.detach() for n, t in osd.items() if t.grad is not None}
    grads.update(extra)
    return {k: v.detach() for k, v in vals.items()}, grads


def rel(a, b):
    """max |a - b| / max(1, max |b|): the project's bound on values"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0))


@functools.lru_cache(maxsize=None)
def module(name):
    """(module, state dict) of a table entry, built once per process"""
    return build(ALL[name] if name in ALL else REFUSED[name][0])


@functools.lru_cache(maxsize=None)
def reference(name, P):
    """float64 oracle of entry `name` at P points and the float32 oracle's own distance from it:
    -> dict(inp, vals, grads, e_vals {key: rel}, e_grads {key: grel})"""
    entry = ALL[name]
    _, sd = module(name)
    inp = inputs(entry, P)
    v64, g64 = oracle_run(entry, sd, inp, torch.float64)
    v32, g32 = oracle_run(entry, sd, inp, torch.float32)
    return dict(inp=inp, vals=v64, grads=g64, e_vals={k: rel(v32[k], v64[k]) for k in v64},
                e_grads={k: grel(g32[k], g64[k]) for k in g64})
