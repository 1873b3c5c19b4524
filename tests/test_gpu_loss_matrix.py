"""The loss kernels against float64 (tests/loss_ref.py), through the C ABI (_lib.call): ssim_patch_kernel and
patch_metric_kernel<1|2|3> (csrc/blend.hip); color_loss_fwd / _sums / _finish / _bwd, step_loss_fwd / _bwd and
blend_loss_prepare / _fwd / _bwd (csrc/rays_embed.hip).

Sizes.  Rays N = 1, 63, 64, 65, 255, 257, 999 and 341 / 342 (3 N = 1023 / 1026, either side of the 1024-thread stride of the
one-workgroup reductions), every one with no mask, a full, an empty, a one-ray and a random mask (n_mask = N while n = 3 N).
Patches: hps 1, 3, 4, 5 (Npx = 9, 49, 81 -- a partly filled second pass of the 64 lanes --, 121) at N = 1, 3, 4, 5, 6, 255, 257
rays of six content classes (uniform, near-equal, flat bright / dark, equal, half 0 half 1, one channel flat), d_out with both
signs and exact zeros.  The blending step at N = 1, 10, 65, 341, 342, 1025 with 0, 1, 3 (k = 0), 4 (k = 1), 10, 0.6 N and N
valid rays.  The other knobs -- three weight sets by value or from the device vector (with garbage by value), the three sums
vectors as five sums or as [nblk, 5] partials with nblk = 1, 17, 1024, 1025, d_total given or NULL, d_extra given (non-zero
in every slot) or NULL -- cycle over those cases; tests/test_loss_ref.py checks on the CPU that every value of every knob
is reached with and without a mask.

Buffers.  Every input lies inside a larger NaN-filled allocation, every output inside a sentinel-filled one that must come
back untouched outside its extent; every tensor stays alive until the test ends.

Bound: layer_ref.hold, err <= min(max(4 e_ref, floor), 1e-3 max|ref|) per tile of 64 rays; a loss scalar is a one-element
tile whose e_ref is the worst of seven fp32 evaluations with the operands permuted and whose floor counts the roundings
between the reduced sums and the output (loss_ref.ROUNDINGS); the patch rows have no floor but two ulp of the L1 / SSD error.
Bit-exact: m and err_masked of the prepare step, k and the
kept count, which d_err entries are zero, the sign of every L1 gradient outside ties, zero gradients where pred == gt and in
the rays whose d_out is zero.  The status word is 0 after every case but the one without a valid ray, whose Lpatch, colour
total and total are NaN as in the reference's mean of an empty selection.  Measured: profiles/r11_loss_matrix.txt
(NUDF_LOSS_REPORT writes it)."""
import os

import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.0
NAN = float("nan")
PAD = 4           # floats (or int64s) of NaN / sentinel on either side of every buffer's extent
_ROWS = []        # (case, output, worst err / e_ref, err, e_ref, bound, tiles, floor)
_KEEP = []        # every tensor a launch was handed, alive until the test ends (the kernels run asynchronously)


@pytest.fixture(scope="module")
def dev():
    from neuraludf_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    _lib.bind_status(d)
    assert _lib.read_status(d, clear=True) >= 0
    yield d
    path = os.environ.get("NUDF_LOSS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("loss matrix against float64: per kernel family and output, the case whose worst tile has the largest err / e_ref\n")
            f.write("(max norm of the tile; tiles = all tiles of all the family's cases); bound = min(max(4 e_ref, floor), 1e-3 max|ref|)\n\n")
            f.write("%-58s %-10s %9s %9s %9s %9s %5s %8s\n" % ("case", "output", "err/e_ref", "err", "e_ref", "bound", "tiles", "floor"))
            worst, ntiles = {}, {}
            for r in _ROWS:
                key = (_family(r[0]), r[1])
                ntiles[key] = ntiles.get(key, 0) + r[6]
                if key not in worst or r[2] > worst[key][2]:
                    worst[key] = r
            for key, r in worst.items():
                f.write("%-58s %-10s %9.2f %9.2e %9.2e %9.2e %5d %8.1e\n" % (r[:6] + (ntiles[key], r[7])))
            by_floor = [r for r in _ROWS if r[3] > R.FACTOR * r[4]]
            f.write("\nrows with err > 4 e_ref, which a floor lets pass: %d of %d\n" % (len(by_floor), len(_ROWS)))
            for r in by_floor:
                f.write("%-58s %-10s err %.2e e_ref %.2e floor %.1e\n" % (r[0], r[1], r[3], r[4], r[7]))


def _family(case):
    """patch_<kind>, color, shards, step, blend"""
    p = case.split("_")
    return "_".join(p[:2]) if p[0] == "patch" else p[0]


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """a launch that faulted leaves the device unusable: end the run there instead of launching the remaining cases"""
    yield
    try:
        torch.cuda.synchronize()
        del _KEEP[:]
    except RuntimeError as e:
        pytest.exit("the device reported an error, no further launches: %s" % e, returncode=3)


class In:
    """an input on the device inside a larger NaN-filled allocation (the int64 permutation: padded with index 0, so that a
    stray read of it cannot become a stray address)"""

    def __init__(self, dev, t, tail=PAD):
        flat = t.detach().reshape(-1)
        fill = NAN if flat.dtype.is_floating_point else 0
        b = torch.full((flat.numel() + PAD + tail,), fill, dtype=flat.dtype)
        b[PAD:PAD + flat.numel()] = flat
        self.buf, self.n = b.to(dev), flat.numel()
        _KEEP.append(self.buf)

    @property
    def p(self):
        return self.buf.data_ptr() + PAD * self.buf.element_size()


class Out:
    """a sentinel-filled device buffer of n floats with PAD more on either side; `get` asserts that those came back untouched"""

    def __init__(self, dev, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENT, device=dev)
        _KEEP.append(self.buf)

    @property
    def p(self):
        return self.buf.data_ptr() + 4 * PAD

    def view(self):
        return self.buf[PAD:PAD + self.n]

    def get(self, what):
        b = self.buf.cpu()
        assert bool((b[:PAD] == SENT).all()) and bool((b[PAD + self.n:] == SENT).all()), "%s: written outside its %d floats" % (what, self.n)
        return b[PAD:PAD + self.n].clone()


def P(dev, t, tail=PAD):
    """pointer of an optional input"""
    return None if t is None else In(dev, t, tail).p


def mask_ptr(dev, mask, n):
    """the pixel mask [N] with NaN up to the n = 3 N floats of the colours behind it: a mask loop that runs to n instead of
    n_mask reads them, inside the allocation"""
    return P(dev, mask, tail=n + PAD)


def check(fails):
    assert not fails, "\n".join(fails[:20])


def status(dev, clear=False):
    from neuraludf_amd import _lib
    return _lib.read_status(dev, clear=clear)


def exact_l1_pattern(what, got, r64, pred, gt, keep):
    """the select of an L1 gradient: the sign of every kept element, zero where pred == gt"""
    got, r64 = got.reshape(-1), r64.reshape(-1)
    assert torch.equal(torch.sign(got[keep]).double(), torch.sign(r64[keep])), what + ": sign pattern"
    assert bool((got[(pred == gt).reshape(-1)] == 0).all()), what + ": non-zero where pred == gt"


def weights_of(dev, wname, mode):
    """-> (the by-value weights, the device vector's pointer or None)"""
    w = R.WEIGHTS[wname]
    if mode == "value":
        return w, None
    return R.GARBAGE, P(dev, R.w_dev_vector(w))


# ------------------------------------------------------------------------------------------------------------------ #
# patch errors
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("hps", R.HPS)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_patch_metric_against_float64(dev, kind, hps):
    from neuraludf_amd._lib import call
    fails = []
    for N in R.PATCH_RAYS:
        c, specs = R.patch_case(hps, N), R.patch_rows(kind, hps, N)
        case = "patch_%s_hps%d_N%d" % (kind, hps, N)
        npx = c["npx"]
        pred, gt, win, d_out = In(dev, c["pred"]), In(dev, c["gt"]), In(dev, c["win"]), In(dev, c["d_out"])
        fwd, both, dp = Out(dev, N), Out(dev, N), Out(dev, N * npx * 3)
        call("nudf_patch_metric", R.KINDS[kind], pred.p, gt.p, win.p, N, npx, fwd.p, None, None)
        call("nudf_patch_metric", R.KINDS[kind], pred.p, gt.p, win.p, N, npx, both.p, d_out.p, dp.p)
        err, grad = both.get(case + " err"), dp.get(case + " d_pred")
        assert torch.equal(fwd.get(case + " err (forward only)"), err)
        if kind == "ssim":
            direct, dpd = Out(dev, N), Out(dev, N * npx * 3)
            call("nudf_ssim_patch", pred.p, gt.p, win.p, N, npx, direct.p, d_out.p, dpd.p)
            assert torch.equal(direct.get(case + " ssim"), err) and torch.equal(dpd.get(case + " ssim d_pred"), grad)
        R.hold_rows(case, specs, dict(err=err, d_pred=grad), _ROWS, fails)
        g3 = grad.reshape(N, npx, 3)
        assert bool((g3[c["zero"]] == 0).all()), case + ": a ray with d_out == 0 has a non-zero gradient"
        if kind == "l1":
            exact_l1_pattern(case, grad, specs["d_pred"]["r64"], c["pred"], c["gt"], c["l1_keep"].reshape(-1))
        if kind in ("l1", "ssd"):                       # equal patches: exactly 0
            eq = torch.tensor([R.CLASSES[r % 6] == "equal" for r in range(N)])
            assert bool((err[eq] == 0).all()), case + ": equal patches"
    assert status(dev) == 0
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# ColorLoss: fwd, bwd, and the sharded sums + finish
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("mkind", R.MASKS)
def test_color_loss_against_float64(dev, mkind):
    from neuraludf_amd._lib import call
    fails = []
    for N, mk, wname, di, mode in [c for c in R.COLOR_CASES if c[1] == mkind]:
        c, mask, specs = R.color_case(N), R.mask_case(N, mk), R.color_rows(N, mk, wname, di)
        case = "color_N%d_%s_%s_d%d_%s" % (N, mk, wname, di, mode)
        n = 3 * N
        cb, cc, gt = In(dev, c["cb"]), In(dev, c["c"]), In(dev, c["gt"])
        mp = mask_ptr(dev, mask, n)
        bv, wdev = weights_of(dev, wname, mode)
        out, den, sums = Out(dev, 3), Out(dev, 1), Out(dev, 3)
        call("nudf_color_loss_fwd", cb.p, cc.p, gt.p, n, mp, N, bv["base"], bv["color"], bv["pixel"], wdev, out.p, den.p)
        call("nudf_color_loss_sums", cb.p, cc.p, gt.p, n, mp, N, sums.p)
        # the backward reads den: the float64 one rounded, so that its own error is measured alone
        den_in = In(dev, specs["den"]["r64"].float().reshape(1))
        d_out = In(dev, torch.tensor(R.D_COLOR[di]))
        dcb, dc = Out(dev, n), Out(dev, n)
        call("nudf_color_loss_bwd", cb.p, cc.p, gt.p, n, den_in.p, bv["base"], bv["color"], bv["pixel"], wdev, d_out.p, dcb.p, dc.p)
        o, s = out.get(case + " out"), sums.get(case + " sums")
        got = dict(total=o[0], Lb=o[1], Lc=o[2], den=den.get(case + " den")[0], sums0=s[0], sums1=s[1], sums2=s[2],
                   d_cb=dcb.get(case + " d_cb"), d_c=dc.get(case + " d_c"))
        R.hold_rows(case, specs, got, _ROWS, fails)
        assert float(s[2]) == (n if mask is None else R.mask_count(N, mk))
        exact_l1_pattern(case + " d_cb", got["d_cb"], specs["d_cb"]["r64"], c["cb"], c["gt"], c["keep_cb"])
        exact_l1_pattern(case + " d_c", got["d_c"], specs["d_c"]["r64"], c["c"], c["gt"], c["keep_c"])
    assert status(dev) == 0
    check(fails)


def test_color_loss_of_two_shards_against_the_whole_batch(dev):
    """color_loss_sums of two shards, added as the all-reduce adds them, then color_loss_finish"""
    from neuraludf_amd._lib import call
    fails = []
    for i, (N, mk, wname) in enumerate(R.SHARD_CASES):
        c, mask, specs = R.color_case(N), R.mask_case(N, mk), R.shard_rows(N, mk, wname)
        case = "shards_N%d_%s_%s" % (N, mk, wname)
        cut = N // 3
        parts = []
        for lo, hi in ((0, cut), (cut, N)):
            s = Out(dev, 3)
            sl = lambda t: In(dev, t[lo:hi].contiguous()).p
            mp = None if mask is None else mask_ptr(dev, mask[lo:hi].contiguous(), 3 * (hi - lo))
            call("nudf_color_loss_sums", sl(c["cb"]), sl(c["c"]), sl(c["gt"]), 3 * (hi - lo), mp, hi - lo, s.p)
            parts.append(s)
        total = In(dev, parts[0].get(case + " sums a") + parts[1].get(case + " sums b"))
        bv, wdev = weights_of(dev, wname, ("value", "dev")[i % 2])
        out, den = Out(dev, 3), Out(dev, 1)
        call("nudf_color_loss_finish", total.p, 0 if mask is None else 1, bv["base"], bv["color"], bv["pixel"], wdev, out.p, den.p)
        o = out.get(case + " out")
        R.hold_rows(case, specs, dict(total=o[0], Lb=o[1], Lc=o[2], den=den.get(case + " den")[0]), _ROWS, fails)
    assert status(dev) == 0
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# the step's loss assembly
# ------------------------------------------------------------------------------------------------------------------ #
def _sums_args(dev, sums, nblk):
    """-> (the `sums` argument, sums_ws, nblk, the Out to read the five written sums from or None)"""
    if nblk == 0:
        return In(dev, sums).p, None, 0, None
    written = Out(dev, 5)
    return written.p, In(dev, sums).p, nblk, written


@pytest.mark.parametrize("mkind", R.MASKS)
def test_step_loss_against_float64(dev, mkind):
    from neuraludf_amd._lib import call
    fails = []
    for N, mk, wname, si, nblk, up, mode in [c for c in R.STEP_CASES if c[1] == mkind]:
        c, mask, specs = R.color_case(N), R.mask_case(N, mk), R.step_rows(N, mk, wname, si, nblk, up)
        case = "step_N%d_%s_%s_s%d_nblk%d_%s_%s" % (N, mk, wname, si, nblk, up, mode)
        n = 3 * N
        cb, cc, gt = In(dev, c["cb"]), In(dev, c["c"]), In(dev, c["gt"])
        mp = mask_ptr(dev, mask, n)
        bv, wdev = weights_of(dev, wname, mode)
        wv = (bv["base"], bv["color"], bv["pixel"], bv["igr"], bv["igr_ns"], bv["sparse"])
        sp, ws, nb, written = _sums_args(dev, R.sums_case(si, nblk), nblk)
        out, den = Out(dev, 8), Out(dev, 1)
        call("nudf_step_loss_fwd", cb.p, cc.p, gt.p, n, mp, N, sp, R.N_RAYS, *wv, wdev, out.p, den.p, ws, nb)
        o = out.get(case + " out")
        got = {"out%d" % k: o[k] for k in range(8)}
        got["den"] = den.get(case + " den")[0]
        assert float(o[7]) == 0.0
        if written is not None:
            s = written.get(case + " sums")
            got.update({"sums%d" % k: s[k] for k in range(5)})
        # backward: den and the five sums as the reference has them, rounded to fp32
        den_in, sums_in = In(dev, specs["den"]["r64"].float().reshape(1)), In(dev, specs["_sums_bwd"])
        d_total = P(dev, torch.tensor([R.D_TOTAL])) if up in ("total", "extra") else None
        d_extra = P(dev, torch.tensor(R.D_EXTRA)) if up in ("extra", "extra_null") else None
        dcb, dc, ds = Out(dev, n), Out(dev, n), Out(dev, 5)
        call("nudf_step_loss_bwd", cb.p, cc.p, gt.p, n, den_in.p, sums_in.p, R.N_RAYS, *wv, wdev, d_total, d_extra, dcb.p, dc.p, ds.p)
        got.update(d_cb=dcb.get(case + " d_cb"), d_c=dc.get(case + " d_c"))
        s = ds.get(case + " d_sums")
        got.update({"d_sums%d" % k: s[k] for k in range(5)})
        R.hold_rows(case, specs, got, _ROWS, fails)
        exact_l1_pattern(case + " d_cb", got["d_cb"], specs["d_cb"]["r64"], c["cb"], c["gt"], c["keep_cb"])
        exact_l1_pattern(case + " d_c", got["d_c"], specs["d_c"]["r64"], c["c"], c["gt"], c["keep_c"])
    assert status(dev) == 0
    check(fails)


# ------------------------------------------------------------------------------------------------------------------ #
# the blending step's loss
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("count", R.BLEND_COUNTS)
def test_blend_loss_against_float64(dev, count):
    from neuraludf_amd import _lib
    fails = []
    for N, cnt, wname, si, nblk, d_total in [c for c in R.BLEND_CASES if c[1] == count]:
        c, specs = R.blend_case(N, cnt), R.blend_rows(N, cnt, wname, si, nblk, d_total)
        ref = specs["_ref"]
        case = "blend_N%d_valid%s_%s_s%d_nblk%d_dt%s" % (N, cnt, wname, si, nblk, d_total)
        a = _lib.BlendLoss()
        a.N = N
        m, em = Out(dev, N), Out(dev, N)
        a.err, a.patch_mask, a.weight_sum = In(dev, c["err"]).p, In(dev, c["patch_mask"]).p, In(dev, c["weight_sum"]).p
        a.m, a.err_masked = m.p, em.p
        _lib.call("nudf_blend_loss_prepare", a)
        mh, emh = m.get(case + " m"), em.get(case + " err_masked")
        assert torch.equal(mh, ref["m"].float()), case + ": m"
        assert torch.equal(emh, c["err"] * ref["m"].float()), case + ": err_masked"
        es, order = torch.sort(em.view(), descending=True)              # the caller's sort, on the kernel's own output
        es_in, order_in = In(dev, es.cpu()), In(dev, order.cpu())
        a.cb, a.c, a.pix, a.gt = In(dev, c["cb"]).p, In(dev, c["c"]).p, In(dev, c["pix"]).p, In(dev, c["gt"]).p
        a.err_sorted, a.order = es_in.p, order_in.p
        sp, ws, nb, written = _sums_args(dev, R.sums_case(si, nblk), nblk)
        a.sums, a.sums_ws, a.sums_nblk = sp, ws, nb
        a.w_dev = P(dev, R.w_dev_vector(R.WEIGHTS[wname]))
        out = Out(dev, 12)
        a.out, a.n_rays, a.trim_ratio = out.p, R.N_RAYS, R.RATIO
        _lib.call("nudf_blend_loss_fwd", a)
        o = out.get(case + " out")
        got = {"out%d" % k: o[k] for k in range(12)}
        got.update(m=mh, err_masked=emh)
        if written is not None:
            s = written.get(case + " sums")
            got.update({"sums%d" % k: s[k] for k in range(5)})
        assert float(o[10]) == ref["k"] and float(o[11]) == ref["kept"], (case, float(o[10]), float(o[11]), ref["k"], ref["kept"])
        if cnt == "0":
            # the mean of an empty selection: NaN in the reference, NaN here, and the status word says so
            assert specs["_nan"] == ("out0", "out1", "out5")
            assert all(bool(torch.isnan(o[k])) for k in (0, 1, 5)), case
            assert status(dev, clear=True) == _lib.STATUS_NONFINITE_LOSS
        else:
            assert not specs["_nan"] and status(dev) == 0, case
        # backward: reads the forward's out (den_pix, k, the kept count), m, order and the five sums
        a.sums = In(dev, specs["_sums_bwd"]).p
        a.sums_ws, a.sums_nblk = None, 0
        a.d_total = P(dev, None if d_total is None else torch.tensor([d_total]))
        dcb, dc, dpx, derr, ds = Out(dev, 3 * N), Out(dev, 3 * N), Out(dev, 3 * N), Out(dev, N), Out(dev, 5)
        a.d_cb, a.d_c, a.d_pix, a.d_err, a.d_sums = dcb.p, dc.p, dpx.p, derr.p, ds.p
        _lib.call("nudf_blend_loss_bwd", a)
        got.update(d_cb=dcb.get(case + " d_cb"), d_c=dc.get(case + " d_c"), d_pix=dpx.get(case + " d_pix"), d_err=derr.get(case + " d_err"))
        s = ds.get(case + " d_sums")
        got.update({"d_sums%d" % k: s[k] for k in range(5)})
        R.hold_rows(case, specs, got, _ROWS, fails)
        assert torch.equal(got["d_err"] != 0, ref["keep"]), case + ": the kept set"
        for nm in ("cb", "c", "pix"):
            exact_l1_pattern("%s d_%s" % (case, nm), got["d_" + nm], specs["d_" + nm]["r64"], c[nm], c["gt"], c["keep_" + nm])
    assert status(dev) == 0
    check(fails)
