"""GPU: the texture atlas (neuraludf_amd/meshrender.py texture_atlas, bake_texture, shade_textured; csrc/meshtexture.hip)
against the numpy restatement (tests/meshtexture_ref.py) on the scenes of tests/meshraster_scenes.py: the layout exactly,
the texel counts equal, the colours bit for bit where no pow is involved and to one float32 ulp where one is (the rule of
tests/test_gpu_meshraster.py for nudf_meshraster_colour) -- plus the chart corners against color_vertices, affine ramps,
occlusion, the layout's invariants, the detail a texture keeps and vertex colours lose, repeatability, independence of
unwritten memory, the refusals and the CLI."""
import functools
import os

import numpy as np
import pytest
import torch

import meshraster_ref as R
import meshraster_scenes as S
import meshtexture_ref as T
import scratch_poison as SP
from test_gpu_meshraster import ULP32, _dev, _ref

pytestmark = pytest.mark.gpu

RAG_DENSITY = 16.0       # ragged(): five size classes -- the sheet's faces (longest edge ~0.12) fall on both sides of k = 3 | 4
#                          (778 and 25 faces), the odd faces take k = 5, 6 and 7 (one each) -- in 256 x 256 texels
RAG_GAP, RAG_FILL = 0.05, (0.1, 0.2, 0.3)


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _lay(atlas):
    """a GPU Atlas as the restatement's layout dict"""
    return dict(uv=atlas.uv.cpu().numpy(), W=atlas.W, H=atlas.H, cell_face=atlas.cell_face.cpu().numpy(),
                class_off=tuple(atlas.class_off), class_k=tuple(atlas.class_k))


@functools.lru_cache(maxsize=None)
def _ragged():
    """the scene, its reference depth maps, the restatement's layout and synthetic normals, images and fallback colours"""
    v, f, mats, H, W, want, _ = _ref("ragged")
    rng = np.random.default_rng(21)
    nrm = np.stack([np.sin(v[:, 0] * 3.0), np.cos(v[:, 1] * 2.0), -1.0 + 0 * v[:, 0]], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(v=v, f=f, mats=mats, H=H, W=W, depth=want[0], lay=T.layout(v, f, RAG_DENSITY), nrm=nrm,
                f32=rng.random((3, H, W, 3)).astype(np.float32), u8=rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8),
                fallback=rng.random((len(v), 3)).astype(np.float32))


def _equal_layout(atlas, lay):
    assert (atlas.W, atlas.H) == (lay["W"], lay["H"])
    assert tuple(atlas.class_off) == lay["class_off"] and tuple(atlas.class_k) == lay["class_k"]
    _bits(atlas.uv.cpu().numpy(), lay["uv"], "uv")
    _bits(atlas.cell_face.cpu().numpy(), lay["cell_face"], "cell_face")


# ---- 1. the restatement --------------------------------------------------------------------------------------------------
def test_layout_equals_the_restatement():
    from neuraludf_amd import meshrender
    g = _ragged()
    lay = g["lay"]
    n_k = np.bincount(lay["k"], minlength=13)
    assert (n_k > 0).sum() >= 3 and any(n % 2 for n in n_k if n), n_k        # three size classes, one with an odd count
    assert max(lay["W"], lay["H"]) <= 512
    atlas = meshrender.texture_atlas(_dev(g["v"]), _dev(g["f"]), density=RAG_DENSITY)
    assert isinstance(atlas, meshrender.Atlas) and atlas.uv.dtype == torch.float64 and atlas.density == RAG_DENSITY
    assert atlas.cell_face.dtype == torch.int64
    _equal_layout(atlas, lay)
    # float32 vertices are taken to float64 first
    v32 = g["v"].astype(np.float32)
    _equal_layout(meshrender.texture_atlas(_dev(v32), _dev(g["f"]), density=RAG_DENSITY), T.layout(v32, g["f"], RAG_DENSITY))


@pytest.mark.parametrize("images", ["f32", "u8"])
@pytest.mark.parametrize("normals", [False, True])
def test_bake_and_shade_equal_the_restatement(images, normals):
    from neuraludf_amd import meshrender
    g = _ragged()
    v, f, mats, lay, imgs = g["v"], g["f"], g["mats"], g["lay"], g[images]
    dv, df = _dev(v), _dev(f)
    atlas = meshrender.texture_atlas(dv, df, density=RAG_DENSITY)
    kw = dict(normals=_dev(g["nrm"]), power=2.0) if normals else {}
    fallback = g["fallback"] if images == "u8" else None                     # fill with the float images, the mix with uint8
    tex = meshrender.bake_texture(dv, df, atlas, mats, _dev(imgs), min_gap=RAG_GAP, fill=RAG_FILL, view_chunk=2,
                                  fallback=None if fallback is None else _dev(fallback), **kw)
    assert isinstance(tex, meshrender.Texture) and tex.colors.shape == (lay["H"], lay["W"], 3)
    assert tex.colors.dtype == torch.float32 and tex.n_seen.dtype == torch.int32
    rkw = dict(normals=g["nrm"], cam_pos=R.camera_positions(mats), power=2.0) if normals else {}
    want_c, want_n = T.bake(v, f, lay, mats, g["depth"], imgs, min_gap=RAG_GAP, fill=RAG_FILL, fallback=fallback, **rkw)
    got_c, got_n = tex.colors.cpu().numpy(), tex.n_seen.cpu().numpy()
    _bits(got_n, want_n, "n_seen")
    # every branch is taken: no owner, owned and unseen, one view, several views
    assert (want_n == -1).any() and (want_n == 0).sum() > 100 and (want_n == 1).sum() > 100 and (want_n >= 2).sum() > 100
    if normals:
        blended = want_n > 0                                                 # pow enters the blended texels only
        assert np.abs(got_c[blended] - want_c[blended]).max() <= ULP32
        _bits(got_c[~blended], want_c[~blended], "colors of the texels that are not blended")
    else:
        _bits(got_c, want_c, "colors")
    raster = meshrender.rasterize(dv, df, mats, g["H"], g["W"])
    shaded = meshrender.shade_textured(raster, atlas, tex, background=(0.25, 0.5, 0.75))
    assert shaded.shape == (3, g["H"], g["W"], 3) and shaded.dtype == torch.float32
    want_s = T.shade(raster.face.cpu().numpy(), raster.bary.cpu().numpy(), lay, got_c, (0.25, 0.5, 0.75))
    _bits(shaded.cpu().numpy(), want_s, "shaded")                            # no pow in the draw
    assert (raster.face.cpu().numpy() == -1).any()


# ---- 2. against color_vertices -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tilt45", "ridge"])
@pytest.mark.parametrize("power", [1.0, 2.0])
def test_chart_corners_hold_the_bits_of_color_vertices(name, power):
    from neuraludf_amd import meshclean, meshrender
    v, f, mats, H, W, _, _ = _ref(name)
    dv, df = _dev(v), _dev(f)
    imgs = _dev(np.random.default_rng(5).random((1, H, W, 3)).astype(np.float32))
    nrm = meshclean.vertex_normals(dv, df, torch.float64)
    want_c, want_n = meshrender.color_vertices(dv, df, mats, imgs, normals=nrm, power=power, min_gap=S.VIS_GAP)
    atlas = meshrender.texture_atlas(dv, df, density=10.0)                   # 800 faces of the smallest cell: 256 x 128
    assert atlas.W <= 512
    tex = meshrender.bake_texture(dv, df, atlas, mats, imgs, normals=nrm, power=power, min_gap=S.VIS_GAP)
    ij = atlas.uv.long()                                                     # the corners lie on texel centres
    assert torch.equal(ij.double(), atlas.uv)
    got_c, got_n = tex.colors[ij[..., 1], ij[..., 0]], tex.n_seen[ij[..., 1], ij[..., 0]]          # [F, 3, 3], [F, 3]
    assert SP.same_bits(got_c, want_c[df]) and torch.equal(got_n, want_n[df])
    assert int((want_n > 0).sum()) > 300 and float((want_c[df] - 0.5).abs().max()) > 0.1


# ---- 3. affine ramps -----------------------------------------------------------------------------------------------------
def test_texels_and_textured_draw_reproduce_affine_ramps():
    from neuraludf_amd import meshrender
    v, f = S.square(1.0, 2.0)
    H, W, mats = S.SQ_H, S.SQ_W, S.SQ_P
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    coef = ((0.01, 0.005, 0.1), (-0.001, 0.01, 0.2), (0.006, 0.001, 0.05))
    img = np.stack([a * xs + b * ys + c for a, b, c in coef], -1)[None].astype(np.float32)
    vmax = float(np.abs(img).max())
    ulp = 2.0 ** (np.floor(np.log2(vmax)) - 23)                              # one float32 ulp of the largest value
    dv, df = _dev(v), _dev(f)
    atlas = meshrender.texture_atlas(dv, df, density=8.0)                    # both faces in one cell of side 32
    assert (atlas.W, atlas.H) == (32, 32) and atlas.class_k == (5,)
    tex = meshrender.bake_texture(dv, df, atlas, mats, _dev(img), min_gap=0.0)
    lay = _lay(atlas)
    own = T.owners(lay, len(f))
    jj, ii = np.nonzero(own >= 0)
    assert len(jj) == 32 * 32
    b = T.barycentrics(lay["uv"][own[jj, ii]], ii.astype(np.float64), jj.astype(np.float64))
    tri = f[own[jj, ii]]
    p = sum(b[k][:, None] * v[tri[:, k]] for k in range(3))
    scr = np.stack([R.project(p, mats)[0, :, k] for k in range(2)], -1)      # the gutter lies up to 2 pixels outside the square
    assert scr[:, 0].min() > 1 and scr[:, 0].max() < W - 2 and scr[:, 1].min() > 1 and scr[:, 1].max() < H - 2
    ramp = np.stack([a * scr[:, 0] + b_ * scr[:, 1] + c for a, b_, c in coef], -1)
    got = tex.colors.cpu().numpy()[jj, ii]
    assert np.all(tex.n_seen.cpu().numpy() == 1)                             # nothing hides a texel of the one square
    # The four taps are float32 roundings of the ramp, each off by <= 0.5 ulp; their bilinear mix is convex, so it is off by
    # <= 0.5 ulp from the ramp at the point (bilinear interpolation of an affine function is exact); the cast of the result
    # adds <= 0.5 ulp; the ~20 float64 operations (barycentrics, point, projection, weights, mix, C / S with S = 1) add
    # 20 * 2^-53 relative, < 0.001 ulp: 1.001 ulp in all.
    assert np.abs(got - ramp).max() <= 1.001 * ulp
    # the draw from the same camera: per pixel, UV = the mix of the chart corners by float32 barycentrics, each off by <=
    # 2^-25 (0.5 ulp of a value <= 1), so UV is off by <= 3 * 2^-25 * 32 texels; the texture is the ramp along the chart
    # (the square is fronto-parallel: texel -> pixel is affine, 16 pixels on the 26 texels of the shorter leg) up to the 1.001 ulp above, its
    # bilinear sample is convex (<= 1.001 ulp) and exact for the affine part, and the cast adds 0.5 ulp.
    slope = max(abs(a) + abs(b_) for a, b_, _ in coef) * 16.0 / 26.0         # colour per texel, an upper bound
    tol = 3 * 2.0 ** -25 * 32 * slope + (1.001 + 0.5 + 0.001) * ulp
    raster = meshrender.rasterize(dv, df, mats, H, W)
    shaded = meshrender.shade_textured(raster, atlas, tex).cpu().numpy()[0]
    hit = raster.face[0].cpu().numpy() >= 0
    assert hit.sum() == 17 * 17 and np.abs(shaded[hit] - img[0][hit].astype(np.float64)).max() <= tol
    assert np.all(shaded[~hit] == 0)


# ---- 4. occlusion --------------------------------------------------------------------------------------------------------
def test_hidden_texels_take_the_fill_or_the_fallback():
    from neuraludf_amd import meshrender
    v, f = S.two_squares()
    H, W, mats = S.SQ_H, S.SQ_W, S.SQ_P
    dv, df = _dev(v), _dev(f)
    imgs = np.random.default_rng(9).random((1, H, W, 3)).astype(np.float32)
    fill = (0.1, 0.2, 0.3)
    fb = np.random.default_rng(10).random((len(v), 3)).astype(np.float32)
    atlas = meshrender.texture_atlas(dv, df, density=8.0)
    lay = _lay(atlas)
    own = T.owners(lay, len(f))
    jj, ii = np.nonzero((own == 0) | (own == 1))                             # the large square, at depth 2
    b = T.barycentrics(lay["uv"][own[jj, ii]], ii.astype(np.float64), jj.astype(np.float64))
    tri = f[own[jj, ii]]
    p = sum(b[k][:, None] * v[tri[:, k]] for k in range(3))
    px, py = (np.rint(R.project(p, mats)[0, :, k]) for k in range(2))
    # the small square, at depth 1, covers the pixels [12, 20] x [8, 16]: a point whose 3 x 3 window lies inside is hidden
    hidden = (px >= 13) & (px <= 19) & (py >= 9) & (py <= 15)
    clear = (px < 11) | (px > 21) | (py < 7) | (py > 17)
    assert hidden.sum() > 50 and clear.sum() > 300
    plain = meshrender.bake_texture(dv, df, atlas, mats, _dev(imgs), min_gap=0.2, fill=fill)
    n_seen, colors = plain.n_seen.cpu().numpy(), plain.colors.cpu().numpy()
    assert np.all(n_seen[jj, ii][hidden] == 0) and np.all(n_seen[jj, ii][clear] == 1)
    assert np.all(colors[jj, ii][hidden] == np.asarray(fill, dtype=np.float32))
    assert np.all(n_seen[(own == 2) | (own == 3)] == 1)                      # nothing hides the small square
    mixed = meshrender.bake_texture(dv, df, atlas, mats, _dev(imgs), min_gap=0.2, fill=fill, fallback=_dev(fb))
    fb64 = fb.astype(np.float64)
    want = np.stack([(b[0] * fb64[tri[:, 0], c] + b[1] * fb64[tri[:, 1], c]) + b[2] * fb64[tri[:, 2], c]
                     for c in range(3)], -1).astype(np.float32)
    _bits(mixed.colors.cpu().numpy()[jj, ii][hidden], want[hidden], "fallback mix")
    assert torch.equal(mixed.n_seen, plain.n_seen)
    seen = n_seen > 0
    _bits(mixed.colors.cpu().numpy()[seen], colors[seen], "seen texels with a fallback")


def test_the_rear_camera_supplies_the_back_sheet():
    from neuraludf_amd import meshrender
    v, f, mats, H, W, _, _ = _ref("parallel")
    dv, df = _dev(v), _dev(f)
    imgs = np.empty((2, H, W, 3), dtype=np.float32)
    imgs[0], imgs[1] = 0.25, 0.75
    atlas = meshrender.texture_atlas(dv, df, density=10.0)
    assert atlas.W <= 512
    tex = meshrender.bake_texture(dv, df, atlas, mats, _dev(imgs), min_gap=0.2)
    lay = _lay(atlas)
    own = T.owners(lay, len(f))
    jj, ii = np.nonzero(own >= 0)
    b = T.barycentrics(lay["uv"][own[jj, ii]], ii.astype(np.float64), jj.astype(np.float64))
    inside = (b[0] >= 0) & (b[1] >= 0) & (b[2] >= 0)                         # the gutter leaves the sheets at their borders
    front = own[jj, ii] < len(f) // 2
    n_seen, colors = tex.n_seen.cpu().numpy()[jj, ii], tex.colors.cpu().numpy()[jj, ii]
    assert np.all(n_seen[inside] == 1) and inside.sum() > 1000
    assert np.all(colors[inside & front] == np.float32(0.25)) and np.all(colors[inside & ~front] == np.float32(0.75))


# ---- 5. layout invariants ------------------------------------------------------------------------------------------------
def _longest_edges(v, f):
    p = v[f]
    with np.errstate(all="ignore"):
        sq = np.stack([((p[:, (c + 1) % 3] - p[:, (c + 2) % 3]) ** 2).sum(-1) for c in range(3)], -1)
    return sq


@pytest.mark.parametrize("name", ["ragged", "tilt45"])
def test_layout_invariants(name):
    from neuraludf_amd import meshrender
    v, f = _ref(name)[:2]
    density = RAG_DENSITY if name == "ragged" else 25.0                      # tilt45: every face in the class k = 4
    atlas = meshrender.texture_atlas(_dev(v), _dev(f), density=density)
    lay = _lay(atlas)
    W, H, off, ks = lay["W"], lay["H"], lay["class_off"], lay["class_k"]
    assert H in (W, W // 2) and W & (W - 1) == 0
    assert (len(ks) == 1) == (name == "tilt45") and list(ks) == sorted(ks, reverse=True)
    count = np.zeros((H, W), dtype=np.int32)
    face_k, cell = {}, 0
    for c, k in enumerate(ks):
        s = 1 << k
        li, lj = np.meshgrid(np.arange(s), np.arange(s), indexing="xy")
        lower = li + lj <= s - 1
        for e in range((off[c + 1] - off[c]) >> (2 * k)):
            m0 = off[c] + e * 4 ** k
            X, Y = T.even_bits(m0), T.even_bits(m0 >> 1)
            assert X % s == 0 and Y % s == 0 and X + s <= W and Y + s <= H  # inside the atlas, aligned to its side
            for half, fi in enumerate(lay["cell_face"][cell]):
                if fi >= 0:
                    count[Y:Y + s, X:X + s] += lower if half == 0 else ~lower
                    face_k[int(fi)] = k
                    uvf = lay["uv"][fi]
                    assert np.all(uvf >= [X, Y]) and np.all(uvf < [X + s, Y + s])
                    own_half = [T.owner_half(int(a - X), int(b - Y), s) for a, b in uvf]
                    assert own_half == [half] * 3                            # the corners lie on the face's own texels
            cell += 1
    assert cell == len(lay["cell_face"]) and sorted(face_k) == list(range(len(f)))
    assert count.max() == 1                                                  # the owned texel sets are pairwise disjoint
    assert np.array_equal(count == 1, T.owners(lay, len(f)) >= 0)
    # k is monotone in the longest edge (over the faces that have one)
    sq = _longest_edges(v, f)
    live = np.isfinite(sq).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    k_of = np.asarray([face_k[i] for i in range(len(f))])
    by_len = np.argsort(sq.max(1)[live], kind="stable")
    assert np.all(np.diff(k_of[live][by_len]) >= 0) and np.all(k_of[~live] == 3)
    # counter-clockwise, the right angle opposite the longest edge
    uv = lay["uv"]
    a, b = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    assert np.all(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] > 0)
    uv_sq = np.stack([((uv[:, (c + 1) % 3] - uv[:, (c + 2) % 3]) ** 2).sum(-1) for c in range(3)], -1)
    assert np.array_equal(uv_sq.argmax(1)[live], sq[live].argmax(1))         # (argmax: the first maximum, as the rule says)
    assert np.all(np.sort(uv_sq, 1)[:, 0] == np.sort(uv_sq, 1)[:, 1])        # isosceles


def test_size_finds_the_largest_density_and_max_size_refuses():
    from neuraludf_amd import meshrender
    v, f = _ref("ragged")[:2]
    dv, df = _dev(v), _dev(f)
    for N in (256, 512):
        info = {}
        atlas = meshrender.texture_atlas(dv, df, size=N, _info=info)
        assert atlas.W <= N and info["step"] > 0 and atlas.density > 0
        _equal_layout(atlas, T.layout(v, f, atlas.density))
        wider = meshrender.texture_atlas(dv, df, density=atlas.density + info["step"], max_size=1 << 14)
        assert wider.W > N
    with pytest.raises(ValueError, match="density 1000"):
        meshrender.texture_atlas(dv, df, density=1000.0, max_size=512)
    with pytest.raises(ValueError, match="too small"):
        meshrender.texture_atlas(dv, df, size=64)                            # 403 cells of side 8 need 256 x 128


# ---- 6. detail -----------------------------------------------------------------------------------------------------------
def test_a_texture_keeps_the_detail_vertex_colours_lose(capsys):
    from neuraludf_amd import meshrender
    v, f = S.sheet(4, lambda u, w: (u, w, 2.0 + 0 * u))                      # vertices every 4 pixels
    H, W, mats = S.SQ_H, S.SQ_W, S.SQ_P
    ys, xs = np.mgrid[0:H, 0:W]
    img = np.repeat((((xs // 2) + (ys // 2)) % 2).astype(np.float32)[..., None], 3, -1)[None]
    dv, df, dimg = _dev(v), _dev(f), _dev(img)
    atlas = meshrender.texture_atlas(dv, df, density=16.0)
    assert atlas.W <= 512
    tex = meshrender.bake_texture(dv, df, atlas, mats, dimg, min_gap=0.0)
    raster = meshrender.rasterize(dv, df, mats, H, W)
    mask = raster.face >= 0
    mse_texture = meshrender.image_mse(meshrender.shade_textured(raster, atlas, tex), dimg, mask)
    cv, _ = meshrender.color_vertices(dv, df, mats, dimg, min_gap=0.0)
    corners = df[raster.face.clamp(min=0).long()]                            # [1, H, W, 3]
    vertex_render = (raster.bary[..., None] * cv[corners]).sum(-2)
    mse_vertex = meshrender.image_mse(vertex_render, dimg, mask)
    with capsys.disabled():
        print(f"\nmeshtexture detail: image_mse textured {mse_texture:.6g}, vertex colours {mse_vertex:.6g}")
    assert int(mask.sum()) == 17 * 17 and mse_texture < mse_vertex


# ---- 7. repeatability and unwritten memory -------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_whatever_the_scratch_held():
    from neuraludf_amd import meshrender
    g = _ragged()

    def run():
        dv, df = _dev(g["v"]), _dev(g["f"])
        atlas = meshrender.texture_atlas(dv, df, density=RAG_DENSITY)
        sized = meshrender.texture_atlas(dv, df, size=256)
        tex = meshrender.bake_texture(dv, df, atlas, g["mats"], _dev(g["f32"]), normals=_dev(g["nrm"]), power=2.0,
                                      min_gap=RAG_GAP, fill=RAG_FILL, view_chunk=2)
        mixed = meshrender.bake_texture(dv, df, atlas, g["mats"], _dev(g["u8"]), min_gap=RAG_GAP, fallback=_dev(g["fallback"]))
        raster = meshrender.rasterize(dv, df, g["mats"], g["H"], g["W"])
        out = dict(uv=atlas.uv, cell_face=atlas.cell_face, sized_uv=sized.uv, colors=tex.colors, n_seen=tex.n_seen,
                   mixed=mixed.colors, mixed_n=mixed.n_seen, shaded=meshrender.shade_textured(raster, atlas, tex),
                   scalars=torch.tensor([atlas.W, atlas.H, sized.W, sized.H, sized.density, *atlas.class_off, *atlas.class_k],
                                        dtype=torch.float64))
        torch.cuda.synchronize()
        return {k: t.clone() for k, t in out.items()}

    with SP.poisoned(SP.CLEAN):
        clean = run()
    with SP.poisoned(SP.CLEAN):
        again = run()
    assert SP.same_bits_names(clean, again) == []
    for value in SP.POISONS:
        with SP.poisoned(value):
            leg = run()
        assert SP.same_bits_names(leg, clean) == [], SP.label(value)
    torch.cuda.empty_cache()


# ---- 8. empty and refused inputs -----------------------------------------------------------------------------------------
def test_empty_and_refused_inputs():
    from neuraludf_amd import meshrender
    v, f = S.square(1.0, 2.0)
    H, W, mats = S.SQ_H, S.SQ_W, S.SQ_P
    dv, df = _dev(v), _dev(f)
    img = _dev(np.full((1, H, W, 3), 0.75, dtype=np.float32))
    # no faces: an atlas of one texel nobody owns
    empty = meshrender.texture_atlas(dv, df[:0], density=8.0)
    assert (empty.W, empty.H) == (1, 1) and empty.uv.shape == (0, 3, 2) and empty.cell_face.shape == (0, 2)
    assert empty.class_off == (0,) and empty.class_k == ()
    tex = meshrender.bake_texture(dv, df[:0], empty, mats, img, fill=(0.1, 0.2, 0.3))
    assert tex.n_seen.tolist() == [[-1]] and tex.colors.cpu().numpy().tolist() == [[[np.float32(x) for x in (0.1, 0.2, 0.3)]]]
    raster = meshrender.rasterize(dv, df[:0], mats, H, W)
    assert torch.all(meshrender.shade_textured(raster, empty, tex, background=(1.0, 0.0, 0.5))
                     == torch.tensor([1.0, 0.0, 0.5], device=dv.device))
    # no views: every owned texel takes the fill, or the fallback mix
    atlas = meshrender.texture_atlas(dv, df, density=8.0)
    tex = meshrender.bake_texture(dv, df, atlas, mats[:0], img[:0], fill=(0.1, 0.2, 0.3))
    assert torch.all(tex.n_seen == 0) and torch.all(tex.colors == torch.tensor([0.1, 0.2, 0.3], device=dv.device))
    const = torch.full((4, 3), 0.625, device=dv.device)
    tex = meshrender.bake_texture(dv, df, atlas, mats[:0], img[:0], fallback=const)
    assert torch.all(tex.n_seen == 0) and float((tex.colors - 0.625).abs().max()) <= 2.0 ** -23
    assert meshrender.shade_textured(meshrender.rasterize(dv, df, mats[:0], H, W), atlas, tex).shape == (0, H, W, 3)
    other = meshrender.texture_atlas(dv, df[:1], density=8.0)
    for bad in (lambda: meshrender.texture_atlas(dv, df, density=8.0, size=64),
                lambda: meshrender.texture_atlas(dv, df),
                lambda: meshrender.texture_atlas(dv, df, density=0.0),
                lambda: meshrender.texture_atlas(dv, df, density=float("nan")),
                lambda: meshrender.texture_atlas(dv, df, size=0),
                lambda: meshrender.texture_atlas(torch.from_numpy(v), torch.from_numpy(f), density=8.0),
                lambda: meshrender.bake_texture(dv, df, atlas, mats, img.cpu()),                     # another device
                lambda: meshrender.bake_texture(dv, df, atlas, mats, img, fallback=const[:3]),       # the wrong shape
                lambda: meshrender.bake_texture(dv, df, atlas, mats, img, fallback=const.cpu()),
                lambda: meshrender.bake_texture(dv, df, other, mats, img),                           # another mesh's atlas
                lambda: meshrender.bake_texture(dv, df, (atlas.uv, 32, 32), mats, img),
                lambda: meshrender.bake_texture(dv, df, atlas, mats, img, power=-1.0),
                lambda: meshrender.bake_texture(dv, df, atlas, mats, img, fill=(1.0, 2.0)),
                lambda: meshrender.bake_texture(dv, df, atlas, mats, img, view_chunk=0),
                lambda: meshrender.shade_textured(raster, atlas, tex.colors[:16]),
                lambda: meshrender.shade_textured(raster, atlas, tex.colors.double()),
                lambda: meshrender.shade_textured(raster, atlas, tex, background=(1.0,)),
                lambda: meshrender.shade_textured((raster.depth, raster.face, raster.bary), atlas, tex)):
        with pytest.raises(ValueError):
            bad()
    a, b = torch.zeros(2, 3, 3), torch.ones(2, 3, 3)
    mask = torch.tensor([[True, False, False], [False, False, False]])
    assert meshrender.image_mse(a, b) == 1.0 and meshrender.image_mse(a, b * 2, mask) == 4.0
    assert np.isnan(meshrender.image_mse(a, b, torch.zeros(2, 3, dtype=torch.bool)))


# ---- 9. files ------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_obj_triple(tmp_path, capsys):
    from PIL import Image
    from neuraludf_amd import meshing, meshrender
    v, f = S.tilted_sheet(45.0, n=6)
    H, W = S.VIS_H, S.VIS_W
    mats = np.stack([S.pinhole(20.0, 32.0, 24.0), S.pinhole(20.0, 32.0, 24.0, C=(0.3, 0.0, 0.0))])
    imgs = np.random.default_rng(11).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    scan = tmp_path / "dtu" / "scan1"
    os.makedirs(scan / "mask")
    os.makedirs(scan / "image")
    np.savez(scan / "cameras.npz", **{f"world_mat_{i}": P for i, P in enumerate(mats)})
    for i in range(2):
        Image.fromarray(np.full((H, W, 3), 255, dtype=np.uint8)).save(scan / "mask" / f"{i:03d}.png")
        Image.fromarray(imgs[i]).save(scan / "image" / f"{i:03d}.png")
    meshing.write_ply(tmp_path / "in.ply", v, f)
    rv, rf = meshing.read_ply(tmp_path / "in.ply")
    out = tmp_path / "renders"
    rc = meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--dtu-dir", str(tmp_path / "dtu"), "--scan", "1",
                       "--minimal-vis", "0", "--texture", str(tmp_path / "tex.obj"), "--texture-size", "128",
                       "--render", str(out)])
    assert rc == 0 and "texture: 128 x" in capsys.readouterr().out
    for ext in ("obj", "mtl", "png"):
        assert (tmp_path / f"tex.{ext}").exists()
    ov, of, ouv, otex = meshing.read_obj(tmp_path / "tex.obj")
    np.testing.assert_array_equal(ov.astype(np.float32), rv)
    np.testing.assert_array_equal(of, rf)
    # the same atlas and bake through the library
    dv, df = _dev(rv), _dev(rf)
    atlas = meshrender.texture_atlas(dv, df, size=128)
    nrm = meshing.vertex_normals(dv, df, torch.float64)
    fb, _ = meshrender.color_vertices(dv, df, mats, _dev(imgs), normals=nrm)
    tex = meshrender.bake_texture(dv, df, atlas, mats, _dev(imgs), normals=nrm, fallback=fb)
    assert otex.shape == (atlas.H, atlas.W, 3) and otex.dtype == np.uint8
    np.testing.assert_array_equal(otex, meshing._uchar_colors(tex.colors.cpu().numpy()).reshape(otex.shape))
    np.testing.assert_array_equal(ouv * [atlas.W, atlas.H] - 0.5, atlas.uv.cpu().numpy())
    for i in range(2):
        img = np.asarray(Image.open(out / f"texture_{i}.png"))
        assert img.shape == (H, W, 3) and img.any()
    with pytest.raises(SystemExit):
        meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "x.ply"), "--texture", str(tmp_path / "x.obj")])
    with pytest.raises(SystemExit):
        meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "x.ply"), "--texture-size", "64"])
    capsys.readouterr()


def test_extract_udf_mesh_returns_a_texture():
    """the mesher end to end on the initialised UDF network, simplified, textured from a constant image seen from
    z = -2: the mesh of the run without a texture, normalised UVs inside the unit square, the image's constant where a
    view sees the texel"""
    from common import build_modules
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    H, W = 48, 64
    mats = S.pinhole(40.0, 32.0, 24.0, C=(0.0, 0.0, -2.0))[None]
    imgs = torch.full((1, H, W, 3), 0.625, dtype=torch.float32, device="cuda:0")
    udf = build_modules(fields, seed=0)["udf"].to("cuda:0")
    plain = meshing.extract_udf_mesh(udf, 48, simplify_cell=0.2)
    v, f, uv, texture = meshing.extract_udf_mesh(udf, 48, simplify_cell=0.2, texture_from=(mats, imgs), texture_size=512)
    assert np.array_equal(plain[0], v) and np.array_equal(plain[1], f)
    assert uv.shape == (len(f), 3, 2) and uv.dtype == np.float32 and uv.min() > 0 and uv.max() < 1
    assert texture.dtype == np.uint8 and texture.ndim == 3 and texture.shape[1] <= 512 and texture.shape[2] == 3
    assert (texture == 159).all(-1).any()                                    # rint(0.625 * 255) = 159
    with pytest.raises(ValueError):
        meshing.extract_udf_mesh(udf, 48, texture_from=(mats, imgs), color_from=(mats, imgs))
    with pytest.raises(ValueError):
        meshing.extract_udf_mesh(udf, 48, texture_size=512)
