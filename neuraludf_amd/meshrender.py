"""Drawing the extracted mesh on the GPU (csrc/meshraster.hip): a deterministic triangle rasteriser with a depth buffer and
what rests on it.

    maps         rasterize           depth, face index and barycentrics per pixel, from the dataset cameras
    normals      normal_map          per-pixel normals of a raster, interpolated from vertex normals
    occlusion    vertex_visibility   which vertices each view sees, with a depth test (meshclean.view_counts has none)
    colour       color_vertices      vertex colours blended from the source images over the views that see the vertex
    texture      texture_atlas       one chart per face, two to a power-of-two cell, the cells in Morton order
                 bake_texture        the blend of color_vertices per texel of the atlas (csrc/meshtexture.hip)
                 shade_textured      a raster drawn with the texture; image_mse compares it with a photograph
    cameras      dataset_views, camera_positions

Device tensors in, device tensors out.  A view is rows 0..2 of a world matrix P ([n, 4, 4] or [n, 3, 4], float64 on the
host, as in meshclean.view_counts): q = P p, the pixel is q.xy / q.z and the camera depth q.z.  Pixel (x, y) is the sample
point with exactly those integer coordinates, as in the reference, where round(q.xy / q.z) is the pixel.  There is no
near-plane clipping: a face with a vertex at or behind a camera (q.z <= 0, or not finite) is not drawn in that view, and
`_info` reports how many.  Coverage is two-sided with inclusive edges -- the meshes are open surfaces whose winding means
nothing --, depth is perspective-correct, and a depth tie goes to the smaller face index: a pixel on an edge that two
faces share belongs to exactly one of them.  Every step is float64 with integer atomics only and splits its work with
torch's nonzero (ascending): every result is identical from run to run.  include/nudf.h (NudfMeshRaster) states each
kernel operation by operation; tests/meshraster_ref.py restates them in numpy.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .meshclean import _check_mesh

# (view, face) pairs whose clamped pixel box holds more pixels than this are drawn by a wavefront each instead of a thread
# each: a tuning constant, measured on the 512^3 sphere mesh
LARGE_THRESHOLD = 64
MAX_PIXELS = 1 << 31         # H * W: the pixel count of a face's box is an int32


class Raster(NamedTuple):
    """depth [n, H, W] float32: camera depth of the nearest face, +inf where nothing was drawn; face [n, H, W] int32: its
    index, -1 where nothing was drawn; bary [n, H, W, 3] float32: the barycentrics of the pixel in that face (they weight
    faces[face][0..2]), zeros where nothing was drawn"""
    depth: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor


def _check_views(world_mats, n=None):
    """-> proj np.float64 [n_views, 3, 4], rows 0..2 of each matrix"""
    try:
        mats = np.asarray(world_mats.detach().cpu() if isinstance(world_mats, torch.Tensor) else world_mats,
                          dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("world_mats must be an array of [n_views, 4, 4] (or [n_views, 3, 4]) matrices") from None
    if mats.ndim != 3 or mats.shape[1] not in (3, 4) or mats.shape[2] != 4:
        raise ValueError(f"world_mats must be [n_views, 4, 4] or [n_views, 3, 4] (got {tuple(mats.shape)})")
    if n is not None and mats.shape[0] != n:
        raise ValueError(f"world_mats must hold {n} views like the images (got {mats.shape[0]})")
    return np.ascontiguousarray(mats[:, :3, :])


def _check_image_size(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be >= 1 (got {H}, {W})")
    if H * W >= MAX_PIXELS:
        raise ValueError(f"H * W must be < 2^31 (got {H} x {W})")
    return H, W


def _check_chunk(view_chunk):
    view_chunk = int(view_chunk)
    if view_chunk < 1:
        raise ValueError(f"view_chunk must be >= 1 (got {view_chunk})")
    return view_chunk


def camera_positions(world_mats):
    """camera centres of the views -> np.float64 [n_views, 3]: -M^-1 p4 with M the left 3 x 3 block of P and p4 its fourth
    column, on the host in float64 (the point that projects to q = 0)"""
    proj = _check_views(world_mats)
    return np.stack([-np.linalg.inv(P[:, :3]) @ P[:, 3] for P in proj]) if len(proj) else np.zeros((0, 3))


class _Chunk(NamedTuple):
    desc: _lib.MeshRaster
    scr: torch.Tensor          # [c, V, 3] float64
    zbuf: torch.Tensor         # [c, H, W] int64 keys
    keep: tuple                # what the descriptor points at


def _draw_chunk(pos, faces, proj, H, W, large_threshold, info):
    """project, bounds and the two draws of the views `proj` ([c, 3, 4] on the device) -> _Chunk, ready for resolve"""
    dev, c, n_verts, n_faces = pos.device, proj.shape[0], pos.shape[0], faces.shape[0]
    scr = torch.empty((c, n_verts, 3), dtype=torch.float64, device=dev)
    npix = torch.empty((c, n_faces), dtype=torch.int32, device=dev)
    zbuf = torch.full((c, H, W), -1, dtype=torch.int64, device=dev)           # all-ones: nothing drawn
    d = _lib.MeshRaster(pos=ptr(pos), faces=ptr(faces), proj=ptr(proj), scr=ptr(scr), npix=ptr(npix), zbuf=ptr(zbuf),
                        n_faces=n_faces, n_verts=n_verts, n_views=c, H=H, W=W)
    call("nudf_meshraster_project", d)
    call("nudf_meshraster_bounds", d)
    flat = npix.reshape(-1)
    entries = torch.nonzero(flat).reshape(-1)                                 # ascending view * n_faces + f
    big = flat[entries] > large_threshold
    small, large = entries[~big].contiguous(), entries[big].contiguous()
    for name, lst in (("nudf_meshraster_draw_small", small), ("nudf_meshraster_draw_large", large)):
        if lst.numel():
            d.entries, d.n_entries = ptr(lst), lst.numel()
            call(name, d)
    d.entries, d.n_entries = None, 0
    if info is not None:
        valid = torch.isfinite(scr).all(-1) & (scr[..., 2] > 0)              # [c, V]
        if n_faces:
            info["skipped"] += int((~(valid[:, faces[:, 0]] & valid[:, faces[:, 1]] & valid[:, faces[:, 2]])).sum())
        info["small"] += small.numel()
        info["large"] += large.numel()
    return _Chunk(d, scr, zbuf, (pos, faces, proj, npix, small, large))


def _prepare(verts, faces, world_mats, H, W, view_chunk):
    verts, faces = _check_mesh(verts, faces)
    proj = _check_views(world_mats)
    H, W = _check_image_size(H, W)
    return verts.double().contiguous(), faces, torch.from_numpy(proj).to(verts.device), H, W, _check_chunk(view_chunk)


@torch.no_grad()
def rasterize(verts, faces, world_mats, H, W, view_chunk=8, _large_threshold=None, _info=None):
    """draws the mesh into every view -> Raster(depth [n, H, W] float32, face [n, H, W] int32, bary [n, H, W, 3] float32).
    verts [V, 3] float32 or float64 and faces [F, 3] int64 on a GPU, world_mats [n, 4, 4] on the host; see the module
    docstring for the conventions.  `view_chunk` views are drawn at a time, which bounds the 8-byte depth-and-face buffer
    ([view_chunk, H, W]) and the per-view work lists.  Per chunk: project the vertices, count the pixels of every face's
    box, split the faces that draw something into a small list (one thread each) and a large one (one wavefront each;
    `_large_threshold` pixels, default LARGE_THRESHOLD -- the split changes the time only, never the result), draw both
    with a 64-bit atomicMin per covered pixel, resolve.  `_info`: a dict that receives, summed over the views, `skipped`
    (faces not drawn in a view because one of their vertices is at or behind the camera or not finite there), `small`
    and `large` (the lengths of the two lists)."""
    pos, faces, proj, H, W, view_chunk = _prepare(verts, faces, world_mats, H, W, view_chunk)
    thr = LARGE_THRESHOLD if _large_threshold is None else int(_large_threshold)
    if thr < 0:
        raise ValueError(f"_large_threshold must be >= 0 (got {thr})")
    dev, n = pos.device, proj.shape[0]
    info = dict(skipped=0, small=0, large=0) if _info is not None else None
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    face = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    bary = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
    for s in range(0, n, view_chunk):
        ch = _draw_chunk(pos, faces, proj[s:s + view_chunk].contiguous(), H, W, thr, info)
        d = ch.desc
        d.depth, d.face, d.bary = ptr(depth[s:s + view_chunk]), ptr(face[s:s + view_chunk]), ptr(bary[s:s + view_chunk])
        call("nudf_meshraster_resolve", d)
    if _info is not None:
        _info.update(info)
    return Raster(depth, face, bary)


def normal_map(raster, faces, normals):
    """per-pixel normals of a raster -> [n, H, W, 3] float32: the barycentric mix of the vertex normals of the pixel's face,
    sum_k bary[k] * normals[faces[face][k]], normalised; zeros where nothing was drawn or the mix has no length.  normals:
    [V, 3] (meshclean.vertex_normals; orient the faces first).  Torch on the device: no kernel of its own."""
    if not isinstance(raster, Raster):
        raise ValueError("raster must be a Raster (rasterize)")
    if not isinstance(normals, torch.Tensor) or normals.dim() != 2 or normals.shape[1] != 3:
        raise ValueError("normals must be a [V, 3] tensor")
    _, faces = _check_mesh(normals, faces)
    hit = raster.face >= 0
    corners = faces[raster.face.clamp(min=0).long()]                          # [n, H, W, 3]
    mix = (raster.bary[..., None] * normals.float()[corners]).sum(-2)
    length = mix.norm(dim=-1, keepdim=True)
    ok = hit[..., None] & (length > 0) & torch.isfinite(length)
    return torch.where(ok, mix / length.clamp(min=1e-30), torch.zeros_like(mix))


def mean_edge_length(verts, faces):
    """mean length of the 3 F half-edges of the mesh, float64 (NaN for a mesh without faces)"""
    verts, faces = _check_mesh(verts, faces)
    p = verts.double()[faces]                                                  # [F, 3, 3]
    return float((p - p.roll(-1, 1)).norm(dim=-1).mean()) if faces.shape[0] else float("nan")


def _check_gap(min_gap, verts, faces):
    if min_gap is None:
        min_gap = 2.0 * mean_edge_length(verts, faces) if faces.shape[0] else 0.0
    min_gap = float(min_gap)
    if not (min_gap >= 0.0 and np.isfinite(min_gap)):
        raise ValueError(f"min_gap must be finite and >= 0 (got {min_gap})")
    return min_gap


def _visibility(pos, faces, proj, H, W, min_gap, view_chunk):
    dev, n, n_verts = pos.device, proj.shape[0], pos.shape[0]
    vis = torch.zeros((n, n_verts), dtype=torch.uint8, device=dev)
    if n_verts == 0:
        return vis
    for s in range(0, n, view_chunk):
        ch = _draw_chunk(pos, faces, proj[s:s + view_chunk].contiguous(), H, W, LARGE_THRESHOLD, None)
        d = ch.desc
        depth = torch.empty(ch.zbuf.shape, dtype=torch.float32, device=dev)
        d.depth, d.vis, d.min_gap = ptr(depth), ptr(vis[s:s + view_chunk]), min_gap
        call("nudf_meshraster_resolve", d)                                    # face and bary are not needed: NULL
        call("nudf_meshraster_visible", d)
    return vis


@torch.no_grad()
def vertex_visibility(verts, faces, world_mats, H, W, min_gap=None, view_chunk=8):
    """which vertices each view sees -> uint8 [n, V].  A vertex is seen when it is in front of the camera, its pixel
    (round-half-even of its projection) lies inside the image, and float32(z) <= m + float32(min_gap), where z is its
    camera depth and m the largest depth of the mesh's depth map over the 3 x 3 pixels around its pixel (clamped to the
    image; a pixel nothing was drawn into counts as +inf).  On a plane 1 / z is linear in screen coordinates and the
    vertex lies inside the hull of the surrounding pixel centres, so a plane never hides its own vertices at any tilt,
    with no tolerance; `min_gap` is for creases that point away from the camera: the least distance, in camera depth, by
    which an occluder must stand in front.  The rule errs towards "seen".  min_gap=None means twice the mean edge length
    of the mesh: a stated convention (an occluding layer closer than two edges is not told apart from the surface
    itself), not a measured optimum."""
    pos, faces, proj, H, W, view_chunk = _prepare(verts, faces, world_mats, H, W, view_chunk)
    return _visibility(pos, faces, proj, H, W, _check_gap(min_gap, pos, faces), view_chunk)


def _check_colour_args(verts, faces, world_mats, images, normals, power, fill, view_chunk):
    """the argument checks color_vertices and bake_texture share
    -> (verts, faces, proj_np, H, W, view_chunk, power, fill, normals float64 or None)"""
    verts, faces = _check_mesh(verts, faces)
    dev = verts.device
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("images must be a [n_views, H, W, 3] tensor")
    if images.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"images must be uint8 or float32 (got {images.dtype})")
    if images.device != dev:
        raise ValueError(f"images must be on the vertices' GPU (got {images.device})")
    n, H, W = images.shape[:3]
    proj_np = _check_views(world_mats, n)
    H, W = _check_image_size(H, W)
    view_chunk = _check_chunk(view_chunk)
    power = float(power)
    if not (power >= 0.0 and np.isfinite(power)):
        raise ValueError(f"power must be finite and >= 0 (got {power})")
    try:
        fill = [float(x) for x in fill]
    except (TypeError, ValueError):
        raise ValueError(f"fill must be three numbers (got {fill!r})") from None
    if len(fill) != 3:
        raise ValueError(f"fill must be three numbers (got {fill!r})")
    n_verts = verts.shape[0]
    if normals is not None:
        if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != (n_verts, 3) or normals.device != dev:
            raise ValueError(f"normals must be a [{n_verts}, 3] tensor on the vertices' GPU")
        normals = normals.double().contiguous()
    return verts, faces, proj_np, H, W, view_chunk, power, fill, normals


@torch.no_grad()
def color_vertices(verts, faces, world_mats, images, normals=None, power=1.0, min_gap=None, fill=(0.5, 0.5, 0.5),
                   view_chunk=8):
    """vertex colours from the source images -> (colors [V, 3] float32, n_seen [V] int32).  images: [n, H, W, 3] uint8
    (scaled by 1 / 255) or float32 on the vertices' GPU, channels passed through in the order given.  Over the views in
    ascending order that see the vertex (vertex_visibility with `min_gap`): a bilinear sample at its projection, taps
    clamped to the image, weighted by |n . d|^power with `normals` [V, 3] (unit vertex normals, meshclean.vertex_normals)
    and d the unit direction from the vertex to the camera centre (camera_positions) -- the absolute value because an
    open surface has no outside --, or by 1 without normals; colors[v] = sum w c / sum w in float64, n_seen[v] the number
    of those views.  A vertex whose weights sum to 0 (no view sees it, or all see it edge-on) or to nothing finite gets
    `fill` and n_seen 0."""
    verts, faces, proj_np, H, W, view_chunk, power, fill, normals = _check_colour_args(
        verts, faces, world_mats, images, normals, power, fill, view_chunk)
    dev, n, n_verts = verts.device, images.shape[0], verts.shape[0]
    colors = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    n_seen = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    if n_verts == 0:
        return colors, n_seen
    pos = verts.double().contiguous()
    proj = torch.from_numpy(proj_np).to(dev)
    vis = _visibility(pos, faces, proj, H, W, _check_gap(min_gap, pos, faces), view_chunk)
    cam = torch.from_numpy(np.ascontiguousarray(camera_positions(proj_np))).to(dev)
    images = images.contiguous()
    d = _lib.MeshRaster(pos=ptr(pos), proj=ptr(proj), vis=ptr(vis), images=ptr(images), normals=ptr(normals),
                        cam_pos=ptr(cam), colors=ptr(colors), n_seen=ptr(n_seen), n_verts=n_verts, n_views=n, H=H, W=W,
                        image_f32=int(images.dtype == torch.float32), power=power)
    d.fill[0], d.fill[1], d.fill[2] = fill
    call("nudf_meshraster_colour", d)
    return colors, n_seen


# ---- texture atlases (csrc/meshtexture.hip, include/nudf.h nudf_meshtexture_*) ------------------------------------------
ATLAS_K_MIN, ATLAS_K_MAX = 3, 12      # log2 of the smallest and the largest cell side
ATLAS_GUTTER = 6                      # the legs of the charts of a cell of side s are s - 5 and s - 6 texels long
ATLAS_BISECT_ROUNDS = 24              # of texture_atlas(size=N), after the bracket


class Atlas(NamedTuple):
    """uv [F, 3, 2] float64: the corners of every face's chart in texel-centre coordinates (texel (i, j) has its centre
    at (i, j) and is stored at [j, i]; the normalised UV of a point is ((u + 0.5) / W, (v + 0.5) / H)); W, H: the atlas
    size, a power of two and H = W or W / 2; cell_face [n_cells, 2] int64: the faces of the lower and the upper chart of
    every cell in Morton order, -1 = none; class_off: the Morton offset of every size class and the end of the last;
    class_k: log2 of the cell side of every class, descending; density: texels per unit length"""
    uv: torch.Tensor
    W: int
    H: int
    cell_face: torch.Tensor
    class_off: tuple
    class_k: tuple
    density: float


class Texture(NamedTuple):
    """colors [H, W, 3] float32; n_seen [H, W] int32: -1 where no face owns the texel, 0 where no view contributes (the
    texel holds the fill or the fallback mix), else the number of views blended"""
    colors: torch.Tensor
    n_seen: torch.Tensor


def _even_bits(m):
    """the even bits of the int64 tensor m, packed: the x of a Morton index (its y is _even_bits(m >> 1))"""
    m = m & 0x5555555555555555
    for shift, mask in ((1, 0x3333333333333333), (2, 0x0f0f0f0f0f0f0f0f), (4, 0x00ff00ff00ff00ff),
                        (8, 0x0000ffff0000ffff), (16, 0x00000000ffffffff)):
        m = (m | (m >> shift)) & mask
    return m


def _face_edges(pos, faces):
    """-> (longest [F] float64: the length of every face's longest edge, first [F] int64: the corner opposite it, ties
    to the smallest index, small [F] bool: the faces that take the smallest cell whatever the density -- a vertex index
    out of range, a repeated vertex, a squared edge length that is not finite)"""
    n_verts = pos.shape[0]
    in_range = ((faces >= 0) & (faces < n_verts)).all(1)
    tri = pos[faces.clamp(0, max(n_verts - 1, 0))] if n_verts else pos.new_zeros((faces.shape[0], 3, 3))
    d = tri.roll(-1, 1) - tri.roll(-2, 1)                                     # edge c joins the two corners other than c
    sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    first, longest = torch.zeros_like(faces[:, 0]), sq[:, 0]
    for c in (1, 2):
        more = sq[:, c] > longest
        first, longest = torch.where(more, c, first), torch.where(more, sq[:, c], longest)
    repeated = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    return longest.sqrt(), first, ~in_range | repeated | ~torch.isfinite(sq).all(1)


def _face_classes(longest, small, density):
    """k [F] int64: the smallest k in [ATLAS_K_MIN, ATLAS_K_MAX] with 2^k - 6 >= longest * density (the largest when
    there is none), ATLAS_K_MIN where `small`"""
    t = longest * density
    k = torch.full_like(small, ATLAS_K_MIN, dtype=torch.int64)
    for kk in range(ATLAS_K_MIN, ATLAS_K_MAX):
        k = k + (t > float((1 << kk) - ATLAS_GUTTER))
    return torch.where(small, ATLAS_K_MIN, k)


def _atlas_size(counts):
    """counts[i] = the number of faces of class k = ATLAS_K_MAX - i -> (class_k, class_cells, class_off, W, H)"""
    class_k, cells, off = [], [], [0]
    for i, n in enumerate(counts):
        if n:
            class_k.append(ATLAS_K_MAX - i)
            cells.append((n + 1) // 2)
            off.append(off[-1] + cells[-1] * 4 ** class_k[-1])
    W = 1
    while W * W < off[-1]:
        W *= 2
    return class_k, cells, off, W, (W // 2 if 0 < off[-1] <= W * W // 2 else W)


def _class_counts(k):
    return torch.bincount(ATLAS_K_MAX - k, minlength=ATLAS_K_MAX - ATLAS_K_MIN + 1).tolist()


@torch.no_grad()
def texture_atlas(verts, faces, density=None, size=None, max_size=8192, _info=None):
    """a texture atlas of the mesh -> Atlas.  Every face gets a chart of its own, a right isosceles triangle of texels
    whose legs hold at least (longest edge) * `density` texels; two charts share a square cell whose side is a power of
    two between 8 and 4096, and the cells are packed by a prefix sum in Morton order, the largest first: no search, the
    same layout from run to run (include/nudf.h states it rule by rule, tests/meshtexture_ref.py restates it).  A face
    longer than 4090 / density gets the largest cell and is under-sampled.  Inside a cell every chart keeps a gutter:
    the bilinear footprint of any point of a face stays inside the texels that face owns.  `density`: texels per unit
    length; ValueError when the atlas would be wider than `max_size`.  With `size` = N instead, the largest density a
    bisection finds whose atlas is at most N wide: a bracket by doubling from the density at which the longest face
    still fits the smallest cell, then ATLAS_BISECT_ROUNDS halvings; `_info` receives `step`, the width of the last
    bracket (the density found plus `step` does not fit).  Giving both, or neither, is a ValueError."""
    verts, faces = _check_mesh(verts, faces)
    if (density is None) == (size is None):
        raise ValueError("give density or size, not both and not neither")
    max_size = int(max_size)
    if max_size < 1:
        raise ValueError(f"max_size must be >= 1 (got {max_size})")
    dev, n_faces = verts.device, faces.shape[0]
    pos = verts.double().contiguous()
    longest, first, small = _face_edges(pos, faces)
    if size is not None:
        size = int(size)
        if size < 1:
            raise ValueError(f"size must be >= 1 (got {size})")
        limit = min(size, max_size)

        def fits(d):
            return _atlas_size(_class_counts(_face_classes(longest, small, d)))[3] <= limit
        if not fits(0.0):
            raise ValueError(f"size {size} (max_size {max_size}) is too small for {n_faces} faces at any density")
        live = longest[~small]
        top = float(live.max()) if live.numel() else 0.0
        lo = hi = 2.0 / top if top > 0.0 and math.isfinite(2.0 / top) else 1.0      # every face in the smallest cell
        for _ in range(64):                                                          # bracket: hi is the first that does not fit
            hi = 2.0 * lo
            if not math.isfinite(hi) or not fits(hi):
                break
            lo = hi
        if not math.isfinite(hi) or fits(hi):
            hi = lo                                                                  # every density fits (all cells largest)
        for _ in range(ATLAS_BISECT_ROUNDS):
            mid = 0.5 * (lo + hi)
            if not lo < mid < hi:
                break
            if fits(mid):
                lo = mid
            else:
                hi = mid
        density = lo
        if _info is not None:
            _info["step"] = hi - lo
    else:
        try:
            density = float(density)
        except (TypeError, ValueError):
            raise ValueError(f"density must be a number (got {density!r})") from None
        if not (density > 0.0 and math.isfinite(density)):
            raise ValueError(f"density must be finite and > 0 (got {density})")
    k = _face_classes(longest, small, density)
    counts = _class_counts(k)
    class_k, cells, off, W, H = _atlas_size(counts)
    if W > max_size:
        raise ValueError(f"density {density} needs an atlas {W} texels wide, max_size is {max_size}")
    n_cells = sum(cells)
    cell_face = torch.full((n_cells, 2), -1, dtype=torch.int64, device=dev)
    uv = torch.empty((n_faces, 3, 2), dtype=torch.float64, device=dev)
    if n_faces == 0:
        return Atlas(uv, W, H, cell_face, tuple(off), tuple(class_k), density)
    # per class index i = ATLAS_K_MAX - k: where its faces start in the sorted order, its first cell, its Morton offset
    start, cell0, off0, acc, c = [0] * len(counts), [0] * len(counts), [0] * len(counts), 0, 0
    for i, n in enumerate(counts):
        start[i] = acc
        acc += n
        if n:
            cell0[i], off0[i] = sum(cells[:c]), off[c]
            c += 1
    ids = torch.arange(n_faces, dtype=torch.int64, device=dev)
    order = torch.argsort((ATLAS_K_MAX - k) * n_faces + ids)                  # (k descending, face ascending): keys differ
    ci = (ATLAS_K_MAX - k)[order]
    T = lambda lst: torch.tensor(lst, dtype=torch.int64, device=dev)
    rank = ids - T(start)[ci]                                                 # of the face within its class
    slot = 2 * T(cell0)[ci] + rank                                            # cell * 2 + half
    cell_face.view(-1)[slot] = order
    ks = k[order]
    side = torch.ones_like(ks) << ks
    m0 = T(off0)[ci] + (rank >> 1) * (side * side)
    X, Y = _even_bits(m0), _even_bits(m0 >> 1)
    upper = (rank & 1).bool()
    one = torch.ones_like(side)
    lower_c = torch.stack([torch.stack([one, one], -1), torch.stack([side - 4, one], -1),
                           torch.stack([one, side - 4], -1)], 1)                # [F, 3, 2]
    upper_c = torch.stack([torch.stack([side - 2, side - 2], -1), torch.stack([4 * one, side - 2], -1),
                           torch.stack([side - 2, 4 * one], -1)], 1)
    chart = torch.where(upper[:, None, None], upper_c, lower_c) + torch.stack([X, Y], -1)[:, None, :]
    corner = (first[order][:, None] + torch.arange(3, device=dev)) % 3        # chart corner t holds the face's corner
    uv[order[:, None].expand(-1, 3), corner] = chart.double()
    return Atlas(uv, W, H, cell_face, tuple(off), tuple(class_k), density)


def _check_atlas(atlas, faces):
    if not isinstance(atlas, Atlas):
        raise ValueError("atlas must be an Atlas (texture_atlas)")
    if tuple(atlas.uv.shape) != (faces.shape[0], 3, 2) or atlas.uv.dtype != torch.float64 or atlas.uv.device != faces.device:
        raise ValueError(f"atlas.uv must be a [{faces.shape[0]}, 3, 2] float64 tensor on the mesh's GPU: the atlas is of "
                         "another mesh")
    if len(atlas.class_off) != len(atlas.class_k) + 1 or len(atlas.class_k) > ATLAS_K_MAX - ATLAS_K_MIN + 1:
        raise ValueError("atlas.class_off and atlas.class_k do not belong together")


def _atlas_fields(d, atlas):
    """the tx_ fields of a descriptor that describe the layout"""
    d.tx_uv, d.tx_W, d.tx_H = ptr(atlas.uv.contiguous()), atlas.W, atlas.H
    d.tx_cell_face, d.tx_n_cells = ptr(atlas.cell_face), atlas.cell_face.shape[0]
    d.tx_n_classes = len(atlas.class_k)
    cell = 0
    for c, kk in enumerate(atlas.class_k):
        d.tx_class_k[c], d.tx_class_off[c], d.tx_class_cell[c] = kk, atlas.class_off[c], cell
        cell += (atlas.class_off[c + 1] - atlas.class_off[c]) >> (2 * kk)
    d.tx_class_off[len(atlas.class_k)], d.tx_class_cell[len(atlas.class_k)] = atlas.class_off[-1], cell


@torch.no_grad()
def bake_texture(verts, faces, atlas, world_mats, images, normals=None, power=1.0, min_gap=None, fill=(0.5, 0.5, 0.5),
                 fallback=None, view_chunk=8):
    """the texture of `atlas` (texture_atlas of this mesh) from the source images -> Texture(colors [H_a, W_a, 3] float32,
    n_seen [H_a, W_a] int32).  Every texel a face owns is taken to its point on the face, by the barycentrics of the
    texel centre in the face's chart (not clamped: the gutter around a chart continues the face's plane), and coloured
    there as color_vertices colours a vertex, argument for argument: the views in ascending order that see the point
    (the depth test of vertex_visibility with `min_gap`, against the depth maps of all views), bilinear samples weighted
    by |n . d|^power with n the mix of `normals` at the point.  The texel at a chart corner holds exactly the bits
    color_vertices gives that vertex.  A texel no view contributes to takes `fill`, or with `fallback` [V, 3] float32
    (vertex colours, color_vertices) the barycentric mix of its face's fallback colours; a texel no face owns takes
    `fill` and n_seen -1."""
    verts, faces, proj_np, H, W, view_chunk, power, fill, normals = _check_colour_args(
        verts, faces, world_mats, images, normals, power, fill, view_chunk)
    _check_atlas(atlas, faces)
    dev, n, n_verts, n_faces = verts.device, images.shape[0], verts.shape[0], faces.shape[0]
    if fallback is not None:
        if not isinstance(fallback, torch.Tensor) or tuple(fallback.shape) != (n_verts, 3) or fallback.device != dev:
            raise ValueError(f"fallback must be a [{n_verts}, 3] tensor on the vertices' GPU")
        fallback = fallback.float().contiguous()
    pos = verts.double().contiguous()
    proj = torch.from_numpy(proj_np).to(dev)
    min_gap = _check_gap(min_gap, pos, faces)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    for s in range(0, n, view_chunk):
        ch = _draw_chunk(pos, faces, proj[s:s + view_chunk].contiguous(), H, W, LARGE_THRESHOLD, None)
        ch.desc.depth = ptr(depth[s:s + view_chunk])
        call("nudf_meshraster_resolve", ch.desc)                              # face and bary are not needed: NULL
    cam = torch.from_numpy(np.ascontiguousarray(camera_positions(proj_np))).to(dev)
    images = images.contiguous()
    colors = torch.empty((atlas.H, atlas.W, 3), dtype=torch.float32, device=dev)
    n_seen = torch.empty((atlas.H, atlas.W), dtype=torch.int32, device=dev)
    d = _lib.MeshRaster(pos=ptr(pos), faces=ptr(faces), proj=ptr(proj), depth=ptr(depth), images=ptr(images),
                        normals=ptr(normals), cam_pos=ptr(cam), n_faces=n_faces, n_verts=n_verts, n_views=n, H=H, W=W,
                        image_f32=int(images.dtype == torch.float32), power=power, min_gap=min_gap,
                        tx_fallback=ptr(fallback), tx_colors=ptr(colors), tx_n_seen=ptr(n_seen))
    d.fill[0], d.fill[1], d.fill[2] = fill
    _atlas_fields(d, atlas)
    call("nudf_meshtexture_bake", d)
    return Texture(colors, n_seen)


@torch.no_grad()
def shade_textured(raster, atlas, texture, background=(0.0, 0.0, 0.0)):
    """a raster of the atlas's mesh drawn with its texture -> [n, H, W, 3] float32: per pixel the UV of its point, the
    barycentric mix of its face's chart corners, and there a bilinear sample of the texture with taps clamped to the
    atlas; `background` where nothing was drawn.  texture: a Texture or its colors [H_a, W_a, 3] float32."""
    if not isinstance(raster, Raster):
        raise ValueError("raster must be a Raster (rasterize)")
    if not isinstance(atlas, Atlas):
        raise ValueError("atlas must be an Atlas (texture_atlas)")
    tex = texture.colors if isinstance(texture, Texture) else texture
    if (not isinstance(tex, torch.Tensor) or tuple(tex.shape) != (atlas.H, atlas.W, 3) or tex.dtype != torch.float32
            or tex.device != raster.face.device or atlas.uv.device != tex.device):
        raise ValueError(f"texture must be a [{atlas.H}, {atlas.W}, 3] float32 tensor on the raster's GPU")
    try:
        background = [float(x) for x in background]
    except (TypeError, ValueError):
        raise ValueError(f"background must be three numbers (got {background!r})") from None
    if len(background) != 3:
        raise ValueError(f"background must be three numbers (got {background!r})")
    n, H, W = raster.face.shape
    face, bary, tex = raster.face.contiguous(), raster.bary.contiguous(), tex.contiguous()
    out = torch.empty((n, H, W, 3), dtype=torch.float32, device=tex.device)
    d = _lib.MeshRaster(face=ptr(face), bary=ptr(bary), n_faces=atlas.uv.shape[0], n_views=n, H=H, W=W,
                        tx_uv=ptr(atlas.uv.contiguous()), tx_colors=ptr(tex), tx_out=ptr(out), tx_W=atlas.W, tx_H=atlas.H)
    d.tx_background[0], d.tx_background[1], d.tx_background[2] = background
    call("nudf_meshtexture_shade", d)
    return out


def image_mse(a, b, mask=None):
    """mean squared difference of two images [..., H, W, 3] over the pixels where `mask` [..., H, W] is set (all of them
    without a mask), in float64 -> float (NaN when the mask is empty).  Plain torch."""
    d = (a.double() - b.double()) ** 2
    if mask is not None:
        d = d[mask.bool()]
    return float(d.mean()) if d.numel() else float("nan")



def dataset_views(dataset):
    """the cameras and images of a dataset.ray_batch source (RayBatchSource) as this module takes them
    -> (world_mats np.float64 [n, 4, 4], images [n, H, W, 3] on the source's device).  P = K pose^-1 from intrinsics_all
    and pose_all (camera to world), in float64 on the host: the coordinates are those the renderer uses, i.e. the
    normalised box of the mesher before any scale_mat, and the pixel (x, y) of P is the image's [y, x].  The images are
    the source's own float32 tensor: its scale (divided by 256) and channel order (the loader's) pass through."""
    K = dataset.intrinsics_all.detach().cpu().double().numpy()
    pose = dataset.pose_all.detach().cpu().double().numpy()
    return np.stack([k @ np.linalg.inv(p) for k, p in zip(K, pose)]), dataset.images
