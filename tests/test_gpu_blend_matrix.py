"""Every instantiation of the blend kernels (csrc/blend.hip) against float64 (tests/blend_ref.py).

nudf_patch_blend_fwd / _bwd pick patch_blend_kernel<BWD, PC, PB_WAVES>: PC = 2 for (2 hps + 1)^2 > 64 (hps 4, 5), PB_WAVES = 4
for N >= 1024 (else 8); nudf_patch_warp picks patch_warp_kernel<PC> the same way.  Every case runs forward + backward through
models/blend.blend_and_composite, with planar and with channel-interleaved source images:

    hps (Npx)  N     S    V / nl  n_out  background    patch_blend_kernel<fwd & bwd>, and what else the row is there for
    1 (9)      9     3    8 / 10  0      -             <.,1,8>  S < waves: idle waves in the LDS sum
    2 (25)     33    64   8 / 8   0      bg_in         <.,1,8>  nl == V, S a multiple of the wave count, S + n_out = 64
    3 (49)     21    37   8 / 10  5      both          <.,1,8>  ldw > S, S + n_out = 42 (test_gpu_blend.test_blend_stagewise)
    4 (81)     70    13   3 / 10  0      -             <.,2,8>  17 live lanes in chunk 1, V < 8
    5 (121)    21    37   8 / 10  5      both          <.,2,8>  the shipped fine-tune patch size
    5 (121)    1024  7    8 / 10  0      -             <.,2,4>  S not a multiple of 4, N % 4 == 0
    3 (49)     1024  7    10 / 10 0      bg_in         <.,1,4>  V = MAXV = nl
    -          10    64   8 / 10  5      bg_tail       composite only: S + n_out = 69, a 5-lane second pass
    -          7     100  8 / 10  33     both          composite only: S + n_out = 133, a third pass
    -          8     37   5 / 10  5      bg_tail       composite only: N % 4 == 0, V < 8
every row also runs pixel_blend_kernel<false / true> and pixel_composite_kernel<false / true>.  The sample depths reach
0.3 beyond the unit sphere on both sides, so 30 % of the samples take the background side of the inside / background mix.
The 1024-ray cases run the kernels on all rays and hold the 128 of them the reference is evaluated on (first and last
included).  PatchProjector (patch_warp_kernel<1>, <2>, pixel_warp_kernel): hps 3 and 5 at 19 x 23 samples.
(tests/test_blend_ref.py asserts on the CPU that the table reaches all twelve instantiations and the generator's conditions.)

Bound, per case and tensor: err <= min(max(4 e_ref, floor), 1e-3), err = max|a - b| / max|b| against float64 over the rays
none of whose decisions is a tie; e_ref = the same error of the fp32 oracle; floor 1e-5 for values, 1e-4 for gradients
(composite_ref's numbers).  Exact: both image layouts give the same bits; d_logits[..., V:] == 0; the patch launch's
d_w[:, S:] == 0; the warps' masks outside ties.  Measured figures: profiles/r09_blend_matrix.txt."""
import os

import pytest
import torch

import blend_ref as R

pytestmark = pytest.mark.gpu

_ROWS = []        # (case, tensor, err, e_ref, bound, max|ref|)
_TIES = {}        # case -> share of rays (or pixels) left out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield torch.device("cuda:0")
    path = os.environ.get("NUDF_BLEND_REPORT")
    if path:
        _write_report(path)


def _write_report(path):
    with open(path, "w") as f:
        f.write("blend matrix against float64: err = max|gpu - ref64| / max|ref64| over the rays kept, e_ref = the fp32 oracle's\n")
        f.write("bound = min(max(4 e_ref, floor), 1e-3), floor 1e-5 (values) / 1e-4 (gradients)\n\n")
        f.write("%-36s %-13s %9s %9s %9s %9s  %s\n" % ("case", "tensor", "err", "e_ref", "err/e_ref", "bound", "ties left out"))
        worst, by_floor = {}, []
        for case, nm, e, er, bd, mx in _ROWS:
            rt = e / max(er, 1e-300)
            f.write("%-36s %-13s %9.2e %9.2e %9.2f %9.1e  %.4f\n" % (case, nm, e, er, rt, bd, _TIES.get(case, 0.0)))
            if nm not in worst or rt > worst[nm][0]:
                worst[nm] = (rt, case, e, er)
            if e > R.FACTOR * er:
                by_floor.append((case, nm, e, er))
        f.write("\nworst err / e_ref per output kind (4 would pass without a floor)\n")
        for nm, (rt, case, e, er) in worst.items():
            f.write("%-13s %8.2f  %s err %.2e e_ref %.2e\n" % (nm, rt, case, e, er))
        f.write("\nrows with err > 4 e_ref, which the floor lets pass: %d of %d\n" % (len(by_floor), len(_ROWS)))
        for case, nm, e, er in by_floor:
            f.write("%-36s %-13s err %.2e = %.1f e_ref, floor %.0e\n" % (case, nm, e, e / max(er, 1e-300), R.floor_of(nm)))


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_blend_against_float64(dev, idx):
    c, r = R.CASES[idx], R.reference(idx)
    case, full = R.case_id(c), R.make_case(idx)
    print(case, R.instantiations(c), "ties: %d of %d rays" % (int((~r["keep"]).sum()), len(r["keep"])))
    assert float((~r["keep"]).float().mean()) <= R.RAY_TIE_CAP
    _TIES[case] = float((~r["keep"]).float().mean())
    vals, grads = R.launch(dev, full, hwc=False)
    vals_i, grads_i = R.launch(dev, full, hwc=True)
    for a, b in ((vals, vals_i), (grads, grads_i)):
        for nm in a:
            assert (a[nm] is None and b[nm] is None) or torch.equal(a[nm], b[nm]), (nm, "image layouts differ")
    V, S = c["V"], c["S"]
    assert torch.equal(grads["d_logits"][..., V:], torch.zeros_like(grads["d_logits"][..., V:]))
    if c["hps"] is not None and c["n_out"] > 0:
        assert grads["d_w_patch"].shape[1] == S + c["n_out"]
        assert torch.equal(grads["d_w_patch"][:, S:], torch.zeros_like(grads["d_w_patch"][:, S:]))
    fails = []
    R.hold(case, r, vals, grads, _ROWS, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("idx", range(len(R.WARP_CASES)), ids=["hps%d" % c["hps"] for c in R.WARP_CASES])
def test_patch_projector_warps_against_float64(dev, idx):
    """per-view colours on the pixels both sides call valid, masks equal outside ties, both image layouts bit-identical"""
    from neuraludf_amd.models.patch_projector import PatchProjector
    c, r = R.WARP_CASES[idx], R.warp_reference(idx)
    inp, t = r["inp"], r["ties"]
    (p64, pm64, c64, cm64), (p32, _, c32, _) = r["w64"], r["w32"]
    N, S, V, npx = c["N"], c["S"], c["V"], R.npx_of(c["hps"])
    D = lambda x: x.to(dev)
    proj = PatchProjector(c["hps"])
    got = []
    for hwc in (False, True):
        im = D(inp["imgs"])
        if hwc:
            im = im.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        col, msk = proj.pixel_warp(D(inp["pts"]), im, D(inp["intrinsics"]), D(inp["w2cs"]))
        pc, pm = proj.patch_warp(D(inp["pts"]), D(inp["rays_uv"].clone()), D(inp["normals"]), im, D(inp["intrinsics"][0]),
                                 D(inp["intrinsics"]), D(inp["query_c2w"]), D(torch.inverse(inp["w2cs"])))
        assert col.shape == (N, S, V, 3) and msk.shape == (N, S, V) and pc.shape == (N, S, V, npx, 3)
        assert pm.shape == (N, S, V, npx) and pm.dtype == torch.bool
        got.append([x.cpu() for x in (col, msk, pc, pm)])
    for a, b in zip(*got):
        assert torch.equal(a, b), "image layouts differ"
    col, msk, pc, pm = got[0]
    case = "warp_hps%d" % c["hps"]
    _TIES[case] = float(t["patch_pixel"].float().mean())
    assert _TIES[case] <= R.PIXEL_TIE_CAP and float(t["pix"].float().mean()) <= R.RAY_TIE_CAP
    assert not bool(((msk != pm64) & ~t["pix"]).any()), int(((msk != pm64) & ~t["pix"]).sum())
    assert not bool(((pm != cm64) & ~t["patch_pixel"]).any()), int(((pm != cm64) & ~t["patch_pixel"]).sum())
    fails = []
    for nm, a, b32, b64, ok in (("pixel_warp", col, p32, p64, pm64 & msk & ~t["pix"]),
                                ("patch_warp", pc, c32, c64, cm64 & pm & ~t["patch_pixel"])):
        e, er = R.error(a[ok], b64[ok]), R.error(b32[ok], b64[ok])
        bd = R.bound(nm, er)
        print("%s %-12s err %.2e e_ref %.2e bound %.1e" % (case, nm, e, er, bd))
        _ROWS.append((case, nm, e, er, bd, float(b64[ok].abs().max())))
        if not e <= bd:
            fails.append("%s %s: err %.3e > bound %.1e (e_ref %.2e)" % (case, nm, e, bd, er))
    assert not fails, "\n".join(fails)


def test_refusals(dev):
    """V = 11, V > nl and hps = 6 raise NudfError: the launchers return the refusal before their hipLaunchKernelGGL (through
    blend_and_composite the pixel launcher refuses the view counts first, so the patch launcher is also called alone), and
    the device runs the next case as before"""
    from neuraludf_amd import _lib, synth
    from neuraludf_amd.models import blend
    from neuraludf_amd.models.patch_projector import PatchProjector
    full = R.make_case(0)
    D = lambda x: x.to(dev)
    N, S = full["N"], full["S"]

    def run(hps, V, nl, through_patch):
        src = synth.make_source_views(synth.make_scene("tiny"), 0, V)
        imgs = torch.rand(V, 3, full["H"], full["W"])
        logits = torch.randn(N, S, nl)
        args = (D(full["pts"]), D(logits), D(full["w"]), D(full["grad"]), D(full["rays_d"]), D(imgs), D(src["w2cs"]),
                D(src["intrinsics"]), D(src["query_c2w"]), D(full["rays_uv"].clone()))
        if not through_patch:
            return blend.blend_and_composite(hps, *args)
        pts, lg, w, grad, rd, im, w2cs, intr, qc2w, uv = args
        ref_cam, src_cam = blend.patch_cameras(intr[0], intr, qc2w, torch.inverse(w2cs))
        return blend._PatchBlendFn.apply(pts, grad, rd, uv, lg, w, ref_cam, src_cam, im, hps)

    for hps, V, nl in ((1, 11, 11), (1, 8, 6), (6, 8, 10)):
        for through_patch in (False, True):
            with pytest.raises(_lib.NudfError) as ei:
                run(hps, V, nl, through_patch)
            if through_patch:
                assert "V <= 10" in str(ei.value) and "h_patch_size <= 5" in str(ei.value)
    with pytest.raises(_lib.NudfError):
        PatchProjector(6).patch_warp(D(full["pts"]), D(full["rays_uv"].clone()), D(full["grad"]), D(full["imgs"]),
                                     D(full["intrinsics"][0]), D(full["intrinsics"]), D(full["query_c2w"]),
                                     D(full["src_c2ws"]))
    src11 = synth.make_source_views(synth.make_scene("tiny"), 0, 11)
    with pytest.raises(_lib.NudfError):
        PatchProjector(1).pixel_warp(D(full["pts"]), D(torch.rand(11, 3, full["H"], full["W"])), D(src11["intrinsics"]),
                                     D(src11["w2cs"]))
    torch.cuda.synchronize()
    # the device is as it was: the same case still runs and gives the same bits as before
    a = R.launch(dev, full)[0]
    b = R.launch(dev, full)[0]
    assert all(torch.equal(a[k], b[k]) for k in a)
