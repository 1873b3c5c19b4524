"""The per-layer path against float64 (tests/layer_ref.py): every gemm_nn_kernel<EPI>, the per-point kernels of
csrc/rays_embed.hip around it and FusedAdam, through the C ABI (mlp.gemm_nn, _lib.call).

gemm_nn: every variant of layer_ref.VARIANTS (all 13 epilogues with their optional arrays) at (M, N, K) = (1, 1, 32),
(33, 13, 64), (64, 33, 288), (65, 64, 32), (130, 65, 64), (256, 65, 32) [8 block tiles, ragged N: xcd_swizzle permutes],
(512, 130, 64) [24 tiles, tiles_n = 3]; SIGMOID also at N = 3, 6, 35 with iparam = 3.  lda > K, ldb > N, every output and
X array with a leading dimension larger than its extent and a column offset.  A rows >= M, A columns >= K, B columns >= N
and everything of X1 / X2 outside [M, N] hold NaN; every output buffer is pre-filled with a sentinel and must come back
untouched outside [M, N].

Bound, per 32 x 32 tile (64-point block, Adam tensor), max norm: err <= min(max(4 e_ref, floor), 1e-3 max|ref|); e_ref = the
fp32 torch evaluation's distance from float64 on the same tile -- for reductions in an order that is not torch's (the K sum,
signed_colsum, l1_sum, sample_dist) the worst of a few fp32 evaluations with the operands permuted.  Copies, selects, masks
and zeros are bit-exact (their e_ref is 0, so the bound is 0).  Every tile of more than 32 kept elements is held to 4 e_ref
alone.  A floor counts only in tiles of one to 32 elements, where e_ref is the largest of a handful of draws -- ragged edge tiles
of the GEMM and weight-norm rows, a single ray point, the one-element scalar rows -- and for the chain's softplus in the window;
each is derived from the row's arithmetic in layer_ref.py.  Measured, with the rows a floor decided: profiles/r10_layer_matrix.txt.

The softplus window (1e-4 <= exp(100 a) <= 1e-2): the ELEMENT-relative error of SOFTPLUS's C1, of the C1 of
MULSP / TANGENT / BWD / SKIPSPLIT and of udf_grad_seed is at most 4 x the fp32 torch figure of the same quantity
(tests/test_layer_ref.py pins those).  Before the repair of the SOFTPLUS epilogue (log(1 + z) -> log1pf(z)) its C1 was off
by 5.4e-4 there (measured; the same expression with exact exp / log on the CPU: 5.9e-4 at z = 1e-4, test_layer_ref.py)."""
import os

import pytest
import torch

import layer_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.0
NAN = float("nan")
_ROWS = []        # (case, output, worst err / e_ref, err, e_ref, bound, tiles, floor)
_WINDOW = []      # (quantity, element-relative error, fp32 torch figure, bar)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield torch.device("cuda:0")
    path = os.environ.get("NUDF_LAYER_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("layer matrix against float64: per output the tile with the worst err / e_ref (max norm of the tile)\n")
            f.write("bound = min(max(4 e_ref, floor), 1e-3 max|ref|)\n\n")
            f.write("%-40s %-10s %9s %9s %9s %9s %5s %8s\n" % ("case", "output", "err/e_ref", "err", "e_ref", "bound", "tiles", "floor"))
            for r in _ROWS:
                f.write("%-40s %-10s %9.2f %9.2e %9.2e %9.2e %5d %8.1e\n" % r)
            f.write("\nthe softplus window, element-relative\n")
            for r in _WINDOW:
                f.write("%-28s gpu %.3e  torch fp32 %.3e  bar %.3e\n" % r)


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """a launch that faulted leaves the device unusable: end the run there instead of launching the remaining cases"""
    yield
    try:
        torch.cuda.synchronize()
        del _KEEP[:]
    except RuntimeError as e:
        pytest.exit("the device reported an error, no further launches: %s" % e, returncode=3)


_KEEP = []        # every tensor a launch was handed, alive until the test ends (the kernels run asynchronously)


def _ptr(t, off=0):
    from neuraludf_amd._lib import ptr
    if t is None:
        return None
    _KEEP.append(t)
    return ptr(t) + 4 * off


class Out:
    """a sentinel-filled device buffer [rows + 3, width + off + pad]; the kernel is given column `off` of it and the buffer's
    width as the leading dimension (pad = 0: an output without one)"""

    def __init__(self, dev, rows, width, off=0, pad=3, dtype=torch.float32):
        self.rows, self.width, self.off = rows, width, off
        self.buf = torch.full((rows + 3, max(width, 1) + off + pad), SENT, device=dev, dtype=dtype)
        self.ld = self.buf.shape[1]

    @property
    def p(self):
        return _ptr(self.buf, self.off)

    def get(self, what, width=None):
        """the [rows, width] extent on the host; asserts that the rest still holds the sentinel"""
        b = self.buf.cpu()
        w = self.width if width is None else width
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[:self.rows, self.off:self.off + w] = False
        assert bool((b[outside] == SENT).all()), "%s: written outside its [%d, %d] extent" % (what, self.rows, w)
        return b[:self.rows, self.off:self.off + w].clone()


def padded(dev, t, rows=2, cols=3, off=0, fill=NAN):
    """an input on the device inside a larger NaN-filled buffer -> (buffer, ld)"""
    t = t.reshape(t.shape[0], -1)
    b = torch.full((t.shape[0] + rows, t.shape[1] + off + cols), fill, dtype=t.dtype)
    b[:t.shape[0], off:off + t.shape[1]] = t
    return b.to(dev), b.shape[1]


def check(fails):
    assert not fails, "\n".join(fails[:20])


# ------------------------------------------------------------------------------------------------------------------ #
# gemm_nn
# ------------------------------------------------------------------------------------------------------------------ #
def run_gemm(dev, c):
    """launch the case with every array padded / offset -> {"C1": host tensor, ...}"""
    from neuraludf_amd import mlp
    M, N, K, epi, o, r64 = c["M"], c["N"], c["K"], c["epi"], c["o"], c["r64"]
    A, lda = padded(dev, c["A"], rows=3, cols=4)
    ldb = (N + 3) // 4 * 4 + 4
    Bh = torch.full((K, ldb), NAN)
    Bh[:, :N] = c["B"]
    B = Bh.to(dev)
    bias = None if c["bias"] is None else c["bias"].to(dev)
    outs = {}
    for k, v in r64.items():
        if epi == "UDFHEAD" and k != "C1":          # C2 / C3 are [M] vectors: no leading dimension, no offset
            outs[k] = Out(dev, M, 1, off=0, pad=0)
        else:
            outs[k] = Out(dev, M, v.shape[1], off=0 if k == "C3" else 3)
    kw = dict(bias=bias, lda=lda, ldb=ldb, iparam=o.get("iparam", 0), scale=o.get("scale", 1.0), xscale=o.get("xscale", 1.0))
    for k, ob in outs.items():
        kw[k] = ob.buf
        kw["ld" + k.lower()] = ob.ld
        if k != "C3":
            kw[k.lower() + "_off"] = ob.off
        else:
            assert ob.off == 0
    if "apre" in o or "X1" in o:
        x1 = R.stored(o["apre"], o["xscale"]) if "apre" in o else o["X1"]
        kw["X1"], kw["ldx1"] = padded(dev, x1, off=2)
        kw["x1_off"] = 2
    if "X2" in o:
        kw["X2"], kw["ldx2"] = padded(dev, o["X2"], off=1)
        kw["x2_off"] = 1
    mlp.gemm_nn(A, B, M, N, K, epi, **kw)
    torch.cuda.synchronize()
    return {k: ob.get("%s %s" % (epi, k)) for k, ob in outs.items()}


def hold_gemm(case, c, got, fails):
    for k, r64 in c["r64"].items():
        R.hold(case, k, got[k], r64, c["r32"][k], 32, 32, _ROWS, fails, keep=c["keep"], floor=c["floor"][k],
               e_ref_extra=[e[k] for e in c["r32_extra"]])


@pytest.mark.parametrize("name", [v["name"] for v in R.VARIANTS])
def test_gemm_nn_epilogue_against_float64(dev, name):
    var = R.VARIANT[name]
    fails = []
    for si, (M, N, K) in enumerate(var["shapes"]):
        c = R.gemm_case(name, si)
        case = "%s_M%d_N%d_K%d" % (name, M, N, K)
        assert float((~c["keep"]).float().mean()) <= R.TIE_CAP
        got = run_gemm(dev, c)
        hold_gemm(case, c, got, fails)
        o, epi = c["o"], c["epi"]
        # copies and selects are exact
        if epi == "RELU_DUAL" and o.get("c2"):
            assert torch.equal(got["C1"], got["C2"])
        if epi == "SIGMOID" and o.get("c2"):
            assert torch.equal(got["C2"], got["C1"][:, :o["iparam"]])
        if epi in ("MULMASK", "ADDMASK"):
            off = ~(o["X1"] > 0)
            assert bool((got["C1"][off] == 0).all()) and not bool((got["C1"][~off] == 0).any())
        if epi == "UDFHEAD" and o["iparam"] == 0:
            k = c["keep"]
            assert torch.equal(got["C3"][k, 0].double(), torch.sign(c["v64"][k, 0]))
    check(fails)


@pytest.mark.parametrize("epi", ["SOFTPLUS"] + list(R.S_FROM_H))
def test_softplus_window_gemm_nn(dev, epi):
    """element-relative, not tile-relative: the stored h of the window is 1e-6 ... 1e-4, far below the tile's largest"""
    c = R.window_case(epi)
    got = run_gemm(dev, c)
    fails = []
    hold_gemm("window_" + epi, c, got, fails)
    fig = R.relmax(c["r32"]["C1"], c["r64"]["C1"])
    bar = R.WINDOW_FACTOR * fig
    rel = R.relmax(got["C1"], c["r64"]["C1"])
    print("window %s C1: element-relative %.3e, torch fp32 %.3e, bar %.3e" % (epi, rel, fig, bar))
    _WINDOW.append(("gemm_nn %s C1" % epi, rel, fig, bar))
    check(fails)
    assert rel <= bar, "%s C1 is off by %.3e of the element in the softplus window (bar %.3e)" % (epi, rel, bar)


def test_softplus_window_chain_is_recorded(dev):
    """the chain kernels' softplus is log(1 + exp2(-|t|)) on the hardware transcendentals: accurate in absolute terms by
    design, h exactly 0 below a = -0.166.  The same window through a one-step SOFTPLUS chain: the tile bound
    is asserted, the element-relative figure only recorded."""
    from neuraludf_amd import mlp
    c = R.window_case("SOFTPLUS")
    M, N, K = c["M"], c["N"], c["K"]
    assert M == mlp.pad_rows(M) and N == mlp.pad32(N) and K == mlp.k8(K)
    A, B = c["A"].to(dev), c["B"].to(dev)
    C1 = torch.full((M, N), SENT, device=dev)
    cb = mlp.ChainBuilder(M, "LOAD", K)
    cb.init_load(A, K)
    cb.step("SOFTPLUS", mlp.pack_frag(B, N, K, N), K, N, C1=C1, scale=1.0)        # (fp32 fragments: exact products)
    cb.launch()
    torch.cuda.synchronize()
    got = C1.cpu()
    fails = []
    R.hold("window_chain_SOFTPLUS", "C1", got, c["r64"]["C1"], c["r32"]["C1"], 32, 32, _ROWS, fails, floor=R.CHAIN_SOFTPLUS_FLOOR,
           floor_all=True)
    rel = R.relmax(got, c["r64"]["C1"])
    print("window chain SOFTPLUS C1: element-relative %.3e (recorded, not asserted)" % rel)
    _WINDOW.append(("chain SOFTPLUS C1 (recorded)", rel, R.relmax(c["r32"]["C1"], c["r64"]["C1"]), float("nan")))
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# sampling
# ------------------------------------------------------------------------------------------------------------------ #
def _rays(N, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(N, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -2.5])
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    near = 1.5 + 0.2 * torch.rand(N, 1, generator=g)
    far = 3.5 + 0.2 * torch.rand(N, 1, generator=g)
    return o, d, near, far, torch.rand(N, 1, generator=g), g


def _ns(P, S):
    return max(1, (P + S - 1) // S)


@pytest.mark.parametrize("S", [2, 3, 64, 65])
def test_coarse_z_and_coarse_start_against_float64(dev, S):
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        N = _ns(P, S)
        for stride, jitter, center in ((1, True, True), (1, True, False), (1, False, False), (0, True, True)):
            o, d, near, far, t_rand, g = _rays(N, 11 * P + S)
            if stride == 0:
                near, far = near[:1].contiguous(), far[:1].contiguous()
            tr = t_rand if jitter else None
            case = "coarse_S%d_N%d_nf%d_j%d_c%d" % (S, N, stride, jitter, center)
            (z64, sd64), (z32, sd32) = R.coarse_z(near, far, S, tr, center, R.F64), R.coarse_z(near, far, S, tr, center, R.F32)
            z64, z32 = z64.expand(N, S), z32.expand(N, S)
            sd_perm = [R.sample_dist_permuted(near, far, S, torch.randperm(near.shape[0], generator=g)) for _ in range(4)]
            D = lambda t: None if t is None else t.contiguous().to(dev)
            nd, fd, od, dd = D(near), D(far), D(o), D(d)
            # coarse_start: jitter centred inside the kernel, points of mode 0 in the same launch
            z, sd, pts = Out(dev, N, S, pad=0), Out(dev, 1, 1, pad=0), Out(dev, N * S, 3, pad=0)      # (rows are contiguous)
            call("nudf_coarse_start", _ptr(nd), _ptr(fd), stride, _ptr(D(tr)), int(center), N, S, z.p, sd.p, _ptr(od), _ptr(dd), pts.p)
            zg = z.get(case + " z")
            R.hold(case, "z", zg.reshape(-1), z64.reshape(-1), z32.reshape(-1), 64, None, _ROWS, fails)
            R.hold(case, "sdist", sd.get(case + " sd"), sd64, sd32, 1, None, _ROWS, fails, e_ref_extra=sd_perm)
            p64, p32 = R.ray_points(o, d, z64, sd64, 0, R.F64), R.ray_points(o, d, z32, sd32, 0, R.F32)
            R.hold(case, "pts", pts.get(case + " pts"), p64, p32, 64, None, _ROWS, fails, floor=R.ray_floor(o, p64))
            # coarse_z: the caller centres the jitter
            z2, sd2 = Out(dev, N, S, pad=0), Out(dev, 1, 1, pad=0)
            trc = None if tr is None else ((tr.double() - 0.5).float() if center else tr)
            (y64, _), (y32, _) = R.coarse_z(near, far, S, trc, False, R.F64), R.coarse_z(near, far, S, trc, False, R.F32)
            call("nudf_coarse_z", _ptr(nd), _ptr(fd), stride, _ptr(D(trc)), N, S, z2.p, sd2.p)
            R.hold(case, "z(cz)", z2.get(case + " z2").reshape(-1), y64.expand(N, S).reshape(-1), y32.expand(N, S).reshape(-1), 64, None,
                   _ROWS, fails)
            R.hold(case, "sd(cz)", sd2.get(case + " sd2"), sd64, sd32, 1, None, _ROWS, fails, e_ref_extra=sd_perm)
    check(fails)


def test_outside_z_against_float64(dev):
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        for n_out, stride in ((1, 1), (5, 1), (32, 0)):
            N = _ns(P, n_out)
            _, _, _, far, _, g = _rays(N, 3 * P + n_out)
            if stride == 0:
                far = far[:1].contiguous()
            lin = torch.linspace(1e-3, 1.0 - 1.0 / (n_out + 1.0), n_out)
            z64 = R.outside_z(far, lin, 64, R.F64).expand(N, n_out)
            z32 = R.outside_z(far, lin, 64, R.F32).expand(N, n_out)
            zo = Out(dev, N, n_out, pad=0)
            call("nudf_outside_z", _ptr(far.to(dev)), stride, _ptr(lin.to(dev)), N, n_out, 64, zo.p)
            R.hold("outside_N%d_nout%d_f%d" % (N, n_out, stride), "z_out", zo.get("z_out").reshape(-1), z64.reshape(-1), z32.reshape(-1),
                   64, None, _ROWS, fails)
    check(fails)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ray_points_against_float64(dev, mode):
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        for S in (1, 7):
            N = _ns(P, S)
            o, d, near, far, _, g = _rays(N, 5 * P + S + mode)
            z = torch.sort(near + (far - near) * torch.rand(N, S, generator=g), -1)[0]
            if mode == 2:                               # points inside, on and outside the unit sphere
                o = torch.zeros(N, 3)
                z = torch.sort(0.4 + 1.4 * torch.rand(N, S, generator=g), -1)[0]
            sd = torch.tensor([0.0171])
            if mode == 2 and S == 1:
                z[::3, 0] = 1.0 - 0.0171 / 2                    # (the mid point of the last interval is z + sample_dist / 2)
            p64, p32 = R.ray_points(o, d, z, sd, mode, R.F64), R.ray_points(o, d, z, sd, mode, R.F32)
            if mode == 2 and N * S >= 63:
                r = torch.linalg.norm(R.ray_points(o, d, z, sd, 1, R.F64), dim=-1)
                assert bool((r < 1).any()) and bool((r > 1).any()) and (S > 1 or bool(((r - 1).abs() < 1e-6).any()))
            w = 4 if mode == 2 else 3
            pts = Out(dev, N * S, w, pad=0)
            call("nudf_ray_points", _ptr(o.to(dev)), _ptr(d.contiguous().to(dev)), _ptr(z.contiguous().to(dev)), _ptr(sd.to(dev)), N, S, mode, pts.p)
            R.hold("ray_points_m%d_N%d_S%d" % (mode, N, S), "pts", pts.get("pts"), p64, p32, 64, None, _ROWS, fails,
                   floor=R.ray_floor(o, p64) if mode < 2 else 0.0)
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# encoding
# ------------------------------------------------------------------------------------------------------------------ #
DL = [(3, 4), (3, 6), (3, 10), (4, 10), (3, 15)]
COMBOS = [(1, 1.0), (7, 1.0), (1, 0.37), (7, 0.37)]       # (xdiv, in_scale)


@pytest.mark.parametrize("D,L", DL)
@pytest.mark.parametrize("jvp", [False, True])
def test_posenc_value_and_jvp_against_float64(dev, D, L, jvp):
    from neuraludf_amd._lib import call
    E = D * (2 * L + 1)
    fails = []
    for i, P in enumerate(R.POINTS):
        xdiv, in_scale = COMBOS[(i + L) % 4]
        g = torch.Generator().manual_seed(13 * P + L)
        nx = (P + xdiv - 1) // xdiv
        x = torch.randn(nx, D, generator=g) * 0.8
        v = torch.randn(P, D, generator=g) if jvp else None
        s1, s2 = 1.0, 0.70710678
        two = P != 63                                          # one shape runs with the first destination alone
        xb, xld = padded(dev, x, cols=2)
        d1, d2 = Out(dev, P, E, off=2), Out(dev, P, E, off=0)
        call("nudf_posenc", _ptr(xb), xld, xdiv, _ptr(None if v is None else v.to(dev)), D, L, in_scale, P, d1.p, d1.ld, s1,
             d2.p if two else None, d2.ld, s2)
        case = "posenc%s_D%d_L%d_P%d_div%d_in%.2f" % ("_jvp" if jvp else "", D, L, P, xdiv, in_scale)
        for ob, sc, nm in ((d1, s1, "dst1"), (d2, s2, "dst2")):
            if jvp:
                r64, r32 = R.posenc_jvp(x, v, L, in_scale, xdiv, P, sc, R.F64), R.posenc_jvp(x, v, L, in_scale, xdiv, P, sc, R.F32)
            else:
                r64, r32 = R.posenc(x, L, in_scale, xdiv, P, sc, R.F64), R.posenc(x, L, in_scale, xdiv, P, sc, R.F32)
            if nm == "dst2" and not two:
                assert bool((ob.buf == SENT).all())
                continue
            R.hold(case, nm, ob.get(case + nm), r64, r32, 64, None, _ROWS, fails)
    check(fails)


@pytest.mark.parametrize("D,L", DL)
def test_posenc_vjp_against_float64(dev, D, L):
    from neuraludf_amd._lib import call
    E = D * (2 * L + 1)
    fails = []
    for i, P in enumerate(R.POINTS):
        in_scale = (1.0, 0.37)[(i + L) % 2]
        g = torch.Generator().manual_seed(17 * P + L)
        x = torch.randn(P, D, generator=g) * 0.8
        s1, s2 = torch.randn(P, E, generator=g), torch.randn(P, E, generator=g)
        c1, c2 = 1.0, 0.70710678
        two = P != 65
        xb, xld = padded(dev, x, cols=1)
        b1, ld1 = padded(dev, s1, off=2)
        b2, ld2 = padded(dev, s2, off=0)
        gout = Out(dev, P, D, pad=0)
        call("nudf_posenc_vjp", _ptr(xb), xld, D, L, in_scale, P, _ptr(b1, 2), ld1, c1, _ptr(b2) if two else None, ld2, c2, gout.p)
        args = (x, L, in_scale, s1, c1, s2 if two else None, c2)
        R.hold("posenc_vjp_D%d_L%d_P%d_in%.2f" % (D, L, P, in_scale), "g", gout.get("g"), R.posenc_vjp(*args, R.F64), R.posenc_vjp(*args, R.F32),
               64, None, _ROWS, fails)
    check(fails)


def test_posenc_vjp_refuses_an_encoding_wider_than_96(dev):
    from neuraludf_amd import _lib
    x = torch.zeros(4, 3, device=dev)
    s = torch.zeros(4, 99, device=dev)
    gout = Out(dev, 4, 3, pad=0)
    with pytest.raises(_lib.NudfError):
        _lib.call("nudf_posenc_vjp", _ptr(x), 3, 3, 16, 1.0, 4, _ptr(s), 99, 1.0, None, 0, 0.0, gout.p)      # E = 99
    torch.cuda.synchronize()
    assert bool((gout.buf == SENT).all())


def test_copy_cols(dev):
    """scale 1: a copy, bit for bit; scale != 1: one rounding, the bound"""
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        for sdiv, ncols, scale in ((1, 3, 1.0), (7, 5, 1.0), (7, 3, 0.70710678), (1, 33, 0.37)):
            g = torch.Generator().manual_seed(P + ncols)
            src = torch.randn((P + sdiv - 1) // sdiv, ncols + 2, generator=g)
            sb, lds = padded(dev, src, cols=1)
            dst = Out(dev, P, ncols, off=4)
            call("nudf_copy_cols", _ptr(sb), lds, sdiv, dst.p, dst.ld, ncols, P, scale)
            got = dst.get("copy_cols")
            r64, r32 = R.copy_cols(src, sdiv, ncols, P, scale, R.F64), R.copy_cols(src, sdiv, ncols, P, scale, R.F32)
            if scale == 1.0:
                assert torch.equal(got, r32)
            R.hold("copy_cols_P%d_div%d_n%d_s%.2f" % (P, sdiv, ncols, scale), "dst", got, r64, r32, 64, None, _ROWS, fails)
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# head kernels
# ------------------------------------------------------------------------------------------------------------------ #
def test_udf_grad_seed_against_float64(dev):
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        for C, hscale in ((1, 1.0), (33, 1.4142135), (256, 1.4142135)):
            c = R.seed_case(P, C)
            inv_scale = 0.77
            hb, ldh = padded(dev, R.stored(c["apre"], hscale), off=1)
            out = Out(dev, P, C, off=2)
            call("nudf_udf_grad_seed", _ptr(c["sign"].to(dev)), _ptr(c["wrow"].to(dev)), _ptr(hb, 1), ldh, hscale, P, C, inv_scale,
                 out.p, out.ld)
            args = (c["sign"], c["wrow"], c["apre"], inv_scale)
            R.hold("udf_grad_seed_P%d_C%d" % (P, C), "out", out.get("seed"), R.udf_grad_seed(*args, R.F64), R.udf_grad_seed(*args, R.F32),
                   64, None, _ROWS, fails)
    check(fails)


def test_softplus_window_udf_grad_seed(dev):
    from neuraludf_amd._lib import call
    c = R.window_case("MULSP")
    P, C = c["M"], c["N"]
    apre, hscale, inv_scale = c["o"]["apre"], 1.4142135, 0.77
    g = torch.Generator().manual_seed(3)
    sign, wrow = torch.sign(torch.randn(P, generator=g)), torch.randn(C, generator=g) + 2.0
    hb, ldh = padded(dev, R.stored(apre, hscale))
    out = Out(dev, P, C)
    call("nudf_udf_grad_seed", _ptr(sign.to(dev)), _ptr(wrow.to(dev)), _ptr(hb), ldh, hscale, P, C, inv_scale, out.p, out.ld)
    got = out.get("seed")
    args = (sign, wrow, apre, inv_scale)
    r64, r32 = R.udf_grad_seed(*args, R.F64), R.udf_grad_seed(*args, R.F32)
    keep = sign != 0
    fig = R.relmax(r32[keep], r64[keep])
    rel, bar = R.relmax(got[keep], r64[keep]), R.WINDOW_FACTOR * fig
    print("window udf_grad_seed: element-relative %.3e, torch fp32 %.3e, bar %.3e" % (rel, fig, bar))
    _WINDOW.append(("udf_grad_seed", rel, fig, bar))
    assert rel <= bar


def test_udf_head_bwd(dev):
    """column 0 = sign scale dudf (the bound), the feature columns a copy (bit for bit); dudf and dfeat NULL in turn"""
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        for Fw in (1, 33, 256):
            g = torch.Generator().manual_seed(P + Fw)
            sign = torch.sign(torch.randn(P, generator=g))
            dudf, dfeat = torch.randn(P, generator=g), torch.randn(P, Fw, generator=g)
            fb, ldf = padded(dev, dfeat, off=1)
            for has_u, has_f in ((True, True), (False, True), (True, False)):
                out = Out(dev, P, Fw + 1, off=1)
                call("nudf_udf_head_bwd", _ptr(sign.to(dev)), _ptr(dudf.to(dev)) if has_u else None, _ptr(fb, 1) if has_f else None, ldf,
                     P, Fw, 1.3, out.p, out.ld)
                got = out.get("udf_head_bwd")
                a = (sign, dudf if has_u else None, dfeat if has_f else None, 1.3, P, Fw)
                r64, r32 = R.udf_head_bwd(*a, R.F64), R.udf_head_bwd(*a, R.F32)
                assert torch.equal(got[:, 1:], r32[:, 1:])
                if not has_u:
                    assert bool((got[:, 0] == 0).all())
                R.hold("udf_head_bwd_P%d_F%d_u%d_f%d" % (P, Fw, has_u, has_f), "out", got, r64, r32, 64, None, _ROWS, fails)
    check(fails)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 257])
def test_signed_colsum_against_float64(dev, C):
    """accumulates into a non-zero `out`; the sum over points comes in an order of its own (4 x 64 rows per block, atomics
    across blocks): e_ref = worst of the fp32 evaluation and four with the points permuted"""
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        g = torch.Generator().manual_seed(7 * P + C)
        sign, Rm, out0 = torch.sign(torch.randn(P, generator=g)), torch.randn(P, C, generator=g), torch.randn(C, generator=g)
        rb, ldr = padded(dev, Rm, off=0)
        out = Out(dev, 1, C, off=2)
        out.buf[0, 2:2 + C] = out0.to(dev)
        call("nudf_signed_colsum", _ptr(sign.to(dev)), _ptr(rb), ldr, P, C, 0.7, out.p)
        a = (sign, Rm, 0.7, out0)
        extra = [R.signed_colsum(*a, R.F32, perm=torch.randperm(P, generator=g)) for _ in range(4)]
        R.hold("signed_colsum_P%d_C%d" % (P, C), "out", out.get("colsum").reshape(-1), R.signed_colsum(*a, R.F64), R.signed_colsum(*a, R.F32),
               64, None, _ROWS, fails, e_ref_extra=extra)
    check(fails)


def test_sigmoid_head_bwd_against_float64(dev):
    """every combination of dy / dy_extra / draw NULL; the raw columns a copy and the pad columns up to ldo zeros, bit for bit"""
    from neuraludf_amd._lib import call
    fails = []
    for P in R.POINTS:
        for nsig, nraw, ldo in ((3, 0, 32), (3, 32, 64), (6, 1, 7)):
            g = torch.Generator().manual_seed(P + nsig + nraw)
            y = torch.sigmoid(torch.randn(P, nsig, generator=g) * 3)
            dy, dx, dr = torch.randn(P, nsig, generator=g), torch.randn(P, nsig, generator=g), torch.randn(P, max(nraw, 1), generator=g)
            xb, ldx = padded(dev, dx, off=0)
            rb, ldr = padded(dev, dr, off=0)
            for m in range(8):
                hy, hx, hr = bool(m & 1), bool(m & 2), bool(m & 4)
                out = Out(dev, P, ldo, pad=0)
                call("nudf_sigmoid_head_bwd", _ptr(y.to(dev)), _ptr(dy.to(dev)) if hy else None, _ptr(xb) if hx else None, ldx, nsig,
                     _ptr(rb) if hr else None, ldr, nraw, P, out.p, ldo)
                got = out.get("sigmoid_head_bwd")
                a = (y, dy if hy else None, dx if hx else None, dr[:, :nraw] if hr else None, nraw, ldo)
                r64, r32 = R.sigmoid_head_bwd(*a, R.F64), R.sigmoid_head_bwd(*a, R.F32)
                assert torch.equal(got[:, nsig:], r32[:, nsig:])
                R.hold("sigmoid_head_bwd_P%d_%d_%d_%d_m%d" % (P, nsig, nraw, ldo, m), "out", got, r64, r32, 64, None, _ROWS, fails)
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# weight norm
# ------------------------------------------------------------------------------------------------------------------ #
def _wn_hold(case, L, use_g, use_perm, W, Wt, inv, dv, dg, fails):
    """W / W^T / inv_norm / dv / dg of one layer (host tensors; None = not produced) against the reference"""
    perm = L["perm"] if use_perm else None
    g = L["g"] if use_g else None
    (W64, i64), (W32, i32) = R.wn_pack(L["v"], g, perm, R.F64), R.wn_pack(L["v"], g, perm, R.F32)
    fl = R.wn_floors(L, use_g, perm)
    if not use_g and W is not None:
        assert torch.equal(W, W32)                          # a plain Linear: a (permuted) copy
    for nm, got, a, b in (("W", W, W64, W32), ("Wt", Wt, W64.t(), W32.t()), ("inv_norm", inv, i64, i32)):
        if got is not None and a is not None:
            R.hold(case, nm, got, a, b, 64 if nm == "inv_norm" else 32, 32, _ROWS, fails, floor=fl[nm])
    if dv is not None:
        (dv64, dg64), (dv32, dg32) = R.wn_unpack(L["dWp"], L["v"], g, perm, R.F64), R.wn_unpack(L["dWp"], L["v"], g, perm, R.F32)
        if not use_g:
            assert torch.equal(dv, dv32)
        R.hold(case, "dv", dv, dv64, dv32, 32, 32, _ROWS, fails, floor=fl["dv"])
        if use_g:
            R.hold(case, "dg", dg, dg64, dg32, 64, None, _ROWS, fails, floor=fl["dg"])


def _wn_layer(out, inp, seed, use_perm):
    L = dict(R.wn_layer(out, inp, seed))
    dWp = torch.zeros(out, inp)
    if use_perm:
        dWp[:, L["perm"].long()] = L["dW"]
    else:
        dWp = L["dW"]
    L["dWp"] = dWp
    return L


@pytest.mark.parametrize("out", R.WN_OUT)
def test_weightnorm_pack_and_unpack_against_float64(dev, out):
    """single-layer launches: the pack leaves rows >= out and columns >= in alone (callers pre-zero them), so the sentinel
    must survive there; with and without perm, g, inv_norm, Wt"""
    from neuraludf_amd._lib import call
    fails = []
    for inp in R.WN_IN:
        for use_g, use_perm, use_inv, use_wt in ((True, True, True, True), (True, False, False, False), (False, True, False, True),
                                                 (False, False, False, False)):
            L = _wn_layer(out, inp, 100 * out + inp, use_perm)
            case = "wn_out%d_in%d_g%d_p%d" % (out, inp, use_g, use_perm)
            v, g, perm = L["v"].to(dev), L["g"].to(dev) if use_g else None, L["perm"].to(dev) if use_perm else None
            W, Wt, inv = Out(dev, out, inp, off=0), Out(dev, inp, out, off=0), Out(dev, out, 1, pad=0)
            call("nudf_weightnorm_pack", _ptr(v), _ptr(g), out, inp, _ptr(perm), W.p, W.ld, Wt.p if use_wt else None, Wt.ld,
                 inv.p if (use_inv and use_g) else None)
            inv_h = inv.get("inv_norm") if (use_inv and use_g) else None
            if inv_h is None:
                assert bool((inv.buf == SENT).all())
            if not use_wt:
                assert bool((Wt.buf == SENT).all())
            # the unpack reads inv_norm: the float64 one rounded, so that its own error is measured alone
            dWb, ldw = padded(dev, L["dWp"], cols=5)
            invd = (1.0 / torch.linalg.norm(L["v"].double(), dim=1)).float().to(dev)
            dv, dg = Out(dev, out, inp, pad=0), Out(dev, out, 1, pad=0)
            call("nudf_weightnorm_unpack_grad", _ptr(dWb), ldw, _ptr(v), _ptr(g), _ptr(invd) if use_g else None, out, inp, _ptr(perm),
                 dv.p, dg.p if use_g else None)
            if not use_g:
                assert bool((dg.buf == SENT).all())
            _wn_hold(case, L, use_g, use_perm, W.get("W"), Wt.get("Wt") if use_wt else None, inv_h, dv.get("dv"),
                     dg.get("dg").reshape(-1) if use_g else None, fails)
    check(fails)


@pytest.mark.parametrize("variant", ["all", "none", "mixed"])
def test_weightnorm_multi_layer_tables_against_float64(dev, variant):
    """one launch over a table of five layers whose `out` are no multiples of 32 or 4 (block -> layer in the pack,
    row_start -> layer in the unpack).  all: perm, g, inv_norm and W^T as the table says; none: none of the four; mixed: g
    without inv_norm in the pack, the permutation on the layers the table leaves plain (perm without g among them), W^T on
    every other layer"""
    from neuraludf_amd import _lib
    fails = []
    pa, ua = _lib.PackMulti(), _lib.UnpackMulti()
    keep, layers, rows = [], [], 0
    for li, (out, inp, wn, permuted) in enumerate(R.WN_TABLE):
        use_g = wn and variant != "none"
        use_perm = dict(all=permuted, none=False, mixed=not permuted)[variant]
        use_inv = use_g and variant == "all"
        use_wt = variant == "all" or (variant == "mixed" and li % 2 == 1)
        L = _wn_layer(out, inp, 7000 + li, use_perm)
        v, g, perm = L["v"].to(dev), L["g"].to(dev) if use_g else None, L["perm"].to(dev) if use_perm else None
        W, Wt, inv = Out(dev, out, inp), Out(dev, inp, out), Out(dev, out, 1, pad=0)
        P = pa.layer[li]
        P.v, P.g, P.perm, P.W, P.Wt, P.inv_norm = _ptr(v), _ptr(g), _ptr(perm), W.p, (Wt.p if use_wt else None), (inv.p if use_inv else None)
        P.out, P.in_, P.ldw, P.ldwt, P.nfrag, P.row_start = out, inp, W.ld, Wt.ld, 0, rows
        dWb, ldw = padded(dev, L["dWp"], cols=5)
        invd = (1.0 / torch.linalg.norm(L["v"].double(), dim=1)).float().to(dev)
        db = L["db"].to(dev)
        dv, dg, dbo = Out(dev, out, inp, pad=0), Out(dev, out, 1, pad=0), Out(dev, out, 1, pad=0)
        U = ua.layer[li]
        U.dW, U.v, U.g, U.inv_norm, U.perm, U.dv = _ptr(dWb), _ptr(v), _ptr(g), (_ptr(invd) if use_g else None), _ptr(perm), dv.p
        U.dg, U.db_in, U.db_out = (dg.p if use_g else None), _ptr(db), (dbo.p if (variant == "all" or li % 2) else None)
        U.out, U.in_, U.ldw, U.row_start = out, inp, ldw, rows
        rows += out
        keep += [v, g, perm, dWb, invd, db]
        layers.append((L, use_g, use_perm, use_inv, use_wt, W, Wt, inv, dv, dg, dbo, U.db_out is not None))
    pa.n_layers = ua.n_layers = len(R.WN_TABLE)
    pa.total_rows = ua.total_rows = rows
    _lib.call("nudf_weightnorm_pack_multi", pa)
    _lib.call("nudf_weightnorm_unpack_grad_multi", ua)
    torch.cuda.synchronize()
    for li, (L, use_g, use_perm, use_inv, use_wt, W, Wt, inv, dv, dg, dbo, has_dbo) in enumerate(layers):
        case = "wn_multi_%s_layer%d_%dx%d" % (variant, li, L["v"].shape[0], L["v"].shape[1])
        if not use_wt:
            assert bool((Wt.buf == SENT).all())
        if not use_inv:
            assert bool((inv.buf == SENT).all())
        if not use_g:
            assert bool((dg.buf == SENT).all())
        if has_dbo:
            assert torch.equal(dbo.get("db_out").reshape(-1), L["db"])
        else:
            assert bool((dbo.buf == SENT).all())
        _wn_hold(case, L, use_g, use_perm, W.get("W"), Wt.get("Wt") if use_wt else None, inv.get("inv").reshape(-1) if use_inv else None,
                 dv.get("dv"), dg.get("dg").reshape(-1) if use_g else None, fails)
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# scalars and small losses
# ------------------------------------------------------------------------------------------------------------------ #
def test_scalars_at_their_clamps_against_float64(dev):
    """values (continuous in the parameter) always; the derivative's clamp decision outside the margin.  The cases AT a clamp
    are ties by construction (the last bit of exp(10 p) decides): exactly those 7 of the 30 derivatives are left out"""
    from neuraludf_amd._lib import call
    fails = []
    d_scal = torch.tensor([0.3, -1.7, 0.9])
    n_tied = 0
    cases = [(c, R.BETA_HI) for c in R.SCALAR_CASES] + [(c, 2e6) for c in R.SCALAR_CASES_HI]
    for i, ((var, beta, gamma), hi) in enumerate(cases):
        scal, recip, dpar = Out(dev, 1, 3, pad=0), Out(dev, 1, 2, pad=0), Out(dev, 1, 3, pad=0)
        vd, bd, gd, dd = var.to(dev), beta.to(dev), gamma.to(dev), d_scal.to(dev)
        call("nudf_scalars_fwd", _ptr(vd), _ptr(bd), _ptr(gd), hi, scal.p, recip.p)
        call("nudf_scalars_bwd", _ptr(vd), _ptr(bd), _ptr(gd), hi, _ptr(dd), dpar.p)
        (s64, r64, d64), (s32, r32, d32) = R.scalars(var, beta, gamma, hi, d_scal, R.F64), R.scalars(var, beta, gamma, hi, d_scal, R.F32)
        tied = R.scalar_ties(var, beta, gamma, hi)
        n_tied += int(tied.sum())
        case = "scalars_%d" % i
        for k in range(3):
            R.hold(case, "scal%d" % k, scal.get("scal")[0, k], s64[k], s32[k], 1, None, _ROWS, fails, floor=R.scalar_floor(s64[k]))
            if k < 2:
                R.hold(case, "recip%d" % k, recip.get("recip")[0, k], r64[k], r32[k], 1, None, _ROWS, fails, floor=R.scalar_floor(r64[k]))
            if not bool(tied[k]):
                R.hold(case, "dpar%d" % k, dpar.get("dpar")[0, k], d64[k], d32[k], 1, None, _ROWS, fails, floor=R.scalar_floor(d64[k]))
                assert (float(dpar.get("dpar")[0, k]) == 0.0) == (float(d64[k]) == 0.0)
    assert n_tied == R.SCALAR_TIES and 3 * len(cases) == 30
    check(fails)


def test_l1_sum_against_float64(dev):
    from neuraludf_amd._lib import call
    fails = []
    for n in R.POINTS:
        c = R.l1_case(n)
        pred, gt, d_out = c["pred"], c["gt"], c["d_out"]
        m = pred.numel()
        out, dp = Out(dev, 1, 1, pad=0), Out(dev, 1, m, pad=2)
        pd, gd = pred.to(dev), gt.to(dev)
        call("nudf_l1_sum_fwd", _ptr(pd), _ptr(gd), m, out.p)
        call("nudf_l1_sum_bwd", _ptr(pd), _ptr(gd), m, _ptr(d_out.to(dev)), dp.p)
        (s64, g64), (s32, g32) = R.l1_sum(pred, gt, d_out, R.F64), R.l1_sum(pred, gt, d_out, R.F32)
        g = torch.Generator().manual_seed(n)
        extra = [R.l1_sum(pred, gt, d_out, R.F32, perm=torch.randperm(m, generator=g))[0] for _ in range(4)]
        R.hold("l1_sum_n%d" % n, "sum", out.get("l1"), s64, s32, 1, None, _ROWS, fails, e_ref_extra=extra)
        got = dp.get("d_pred").reshape(-1)
        k = c["keep"]
        assert torch.equal(got[k], g32[k])                       # d_out times -1 / 0 / 1: a select
        assert bool((got[(pred == gt).reshape(-1)] == 0).all())
    check(fails)


def test_sums_errors_against_float64(dev):
    from neuraludf_amd._lib import call
    fails = []
    for i, sums in enumerate(([3.7, 120.0, 0.91, 77.0, 41.5], [0.0, 0.0, 0.0, 0.0, 0.0], [1e-3, 1.0, 5.0, 512.0, 500.0])):
        sums, d_err = torch.tensor(sums), torch.tensor([0.7, -1.1, 0.05])
        err, ds = Out(dev, 1, 3, pad=0), Out(dev, 1, 5, pad=0)
        sd = sums.to(dev)
        call("nudf_sums_errors_fwd", _ptr(sd), 512.0, err.p)
        call("nudf_sums_errors_bwd", _ptr(sd), 512.0, _ptr(d_err.to(dev)), ds.p)
        (e64, g64), (e32, g32) = R.sums_errors(sums, 512.0, d_err, R.F64), R.sums_errors(sums, 512.0, d_err, R.F32)
        eg, dg = err.get("err").reshape(-1), ds.get("d_sums").reshape(-1)
        for k in range(3):
            R.hold("sums_errors_%d" % i, "err%d" % k, eg[k], e64[k], e32[k], 1, None, _ROWS, fails, floor=R.quotient_floor(e64[k]))
        for k in range(5):
            R.hold("sums_errors_%d" % i, "d_sums%d" % k, dg[k], g64[k], g32[k], 1, None, _ROWS, fails, floor=R.quotient_floor(g64[k]))
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# Adam
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dyn", [False, True])
def test_fused_adam_against_float64(dev, dyn):
    """sizes around nudf_adam_chunk() = 1024, three groups (one with other betas and eps), a parameter that joins at step 3,
    gradient magnitudes 1e-9 ... 10 so that eps decides some updates; by-value step scalars and the device-scalar path"""
    from neuraludf_amd import _lib
    from neuraludf_amd.optim import FusedAdam
    assert int(_lib.lib().nudf_adam_chunk()) == 1024
    ps0, grads = R.adam_inputs()
    ps = [p.clone().to(dev).requires_grad_(True) for p in ps0]
    opt = FusedAdam([dict(params=[ps[i] for i in grp["idx"]], lr=grp["lr"], betas=grp["betas"], eps=grp["eps"]) for grp in R.ADAM_GROUPS])
    dynbuf = torch.full((2 * len(ps) + 2,), SENT, device=dev)
    for it in range(R.ADAM_STEPS):
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = R.adam_lr(gi, it)
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and it < R.ADAM_LATE) else grads[it][i].to(dev)
        if dyn and it > R.ADAM_LATE:
            # the launch order is settled: the two per-step numbers of every tensor come from device memory
            vals = opt.dyn_values()
            dynbuf[:len(vals)] = torch.tensor(vals, device=dev)
            opt.dyn_base = dynbuf.data_ptr()
        opt.step()
    torch.cuda.synchronize()
    assert bool((dynbuf[2 * len(ps):] == SENT).all())
    r64, r32 = R.adam_reference(R.F64), R.adam_reference(R.F32)
    fails = []
    for i, n in enumerate(R.ADAM_SIZES):
        R.hold("adam_dyn%d_n%d" % (dyn, n), "p", ps[i].detach().cpu(), r64[i], r32[i], n, None, _ROWS, fails)
    check(fails)
