"""Drawing the extracted mesh on the GPU (csrc/meshraster.hip): a deterministic triangle rasteriser with a depth buffer and
what rests on it.

    maps         rasterize           depth, face index and barycentrics per pixel, from the dataset cameras
    normals      normal_map          per-pixel normals of a raster, interpolated from vertex normals
    occlusion    vertex_visibility   which vertices each view sees, with a depth test (meshclean.view_counts has none)
    colour       color_vertices      vertex colours blended from the source images over the views that see the vertex
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


def dataset_views(dataset):
    """the cameras and images of a dataset.ray_batch source (RayBatchSource) as this module takes them
    -> (world_mats np.float64 [n, 4, 4], images [n, H, W, 3] on the source's device).  P = K pose^-1 from intrinsics_all
    and pose_all (camera to world), in float64 on the host: the coordinates are those the renderer uses, i.e. the
    normalised box of the mesher before any scale_mat, and the pixel (x, y) of P is the image's [y, x].  The images are
    the source's own float32 tensor: its scale (divided by 256) and channel order (the loader's) pass through."""
    K = dataset.intrinsics_all.detach().cpu().double().numpy()
    pose = dataset.pose_all.detach().cpu().double().numpy()
    return np.stack([k @ np.linalg.inv(p) for k, p in zip(K, pose)]), dataset.images
