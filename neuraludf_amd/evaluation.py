"""Chamfer evaluation of meshes on the GPU: the DTU and DeepFashion3D protocols of the reference's
evaluation/eval_dtu_python.py (its `__main__` loop, :205-370) and evaluation/eval_deepfashion_python.py (:62-215), with
their open3d file I/O, Python down-sampling loop and sklearn KD-trees replaced.

    sample      sample_mesh         all vertices, then sample_single_tri's points of every triangle of non-zero area
                                    (csrc/pointcloud.hip tri_count / tri_emit, a torch int64 scan between them)
    shuffle     radius_downsample   a seeded torch permutation (the reference's shuffle is unseeded)
    thin        thin                the reference's greedy radius thinning (radius_neighbors + mask loop) as rounds of a
                                    lexicographically-first maximal independent set (thin_round)
    masks       chamfer_dtu         the ObsMask / bounding-box / ground-plane selection in the reference's mixed precision
    distances   nearest             exact float64 nearest neighbours (kneighbors, n_neighbors=1) by rings of hashed cells
    metrics     chamfer_dtu, chamfer_deepfashion    means below max_dist, precision / recall / F-score, the log file
    files       read_ply / write_points_ply (neuraludf_amd.meshing), load_dtu_obs
    surfaces    MeshIndex, closest_on_mesh, mesh_deviation    the exact distance from points to a triangle mesh and the
                                    two-sided deviation between two meshes (csrc/meshdist.hip): the faces binned by their
                                    boxes into the same hashed cells, the same ring search over them; what
                                    trimesh.proximity.closest_point answers on the CPU.  Not part of the two protocols,
                                    which define sampling and stay as they are
    rays        MeshIndex.cast, cast_rays, contains_points, signed_distance    rays against the same index
                                    (csrc/meshray.hip): first hit, any hit, the number of faces crossed; inside / outside
                                    by crossing parity and the signed distance; what trimesh.ray and Trimesh.contains
                                    answer on the CPU
    crossings   MeshIndex.intersections, self_intersections, mesh_intersections    the pairs of faces that pass through
                                    each other, in one mesh or between two (csrc/meshintersect.hip): filtered orient3d /
                                    orient2d signs over the same index; what MeshLab's "select self intersecting faces",
                                    libigl and pymeshfix answer on the CPU
    winding     MeshIndex.winding, winding_number, contains_points / signed_distance with method="winding"    the
                                    generalised winding number (csrc/meshwinding.hip): a linear octree over the faces,
                                    order-2 far-field expansions, exact solid angles nearby; inside / outside that
                                    survives holes and open sheets; what libigl's fast_winding_number answers on the CPU

Given the permutation, every step is the reference's float64 computation in its operation order, so the points, the
masks and the distances equal a numpy restatement bit for bit (tests/pointcloud_ref.py); only the means are summed in
torch's order.  Mesh units are the caller's: for DTU the mesh must be in world space (millimetres), i.e.
`extract_udf_mesh(..., scale_mat=...)` / `Trainer.extract_udf_mesh(world_space=True, scale_mat=...)`.

Empty inputs: an empty GT cloud, an empty data cloud and (DTU) no data point inside the ObsMask or no GT point above the
plane raise ValueError (sklearn raises there); a mean with no distance below max_dist is NaN, as numpy gives.
Non-finite points raise ValueError before thinning or a nearest-neighbour search (sklearn refuses them too).

    python -m neuraludf_amd.evaluation {dtu,deepfashion} --data X.ply --gt Y.ply [--mode mesh|pcd]
        [--dataset_dir D --scan N] [--downsample_density ...] [--patch_size ...] [--max_dist ...]
        [--visualize_threshold ...] [--vis_out_dir ...] [--no_vis] [--log ...] [--seed 0]
    python -m neuraludf_amd.evaluation deviation --a A.ply --b B.ply [--density D] [--bound B] [--log FILE]
    python -m neuraludf_amd.evaluation intersections --mesh A.ply [--other B.ply] [--out FLAGGED.ply]
    python -m neuraludf_amd.evaluation winding --mesh M.ply (--points P.ply | --grid N) --out W.npy [--beta B] [--orient]
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr

MAX_POINTS = 1 << 28            # largest sampled cloud accepted (24 B per point, plus the index: about 20 GB)
AXIS_CELLS = 1 << 21            # cells per axis of the packed cell key
THIN_CELL_SLACK = 1.0 + 2.0 ** -19   # thinning cell / radius: the 27-cell window survives the rounding of cell coordinates
NEAREST_POINTS_PER_CELL = 16    # target points per occupied cell of the nearest-neighbour index (measured: DESIGN.md §4.9)
MESH_CELL_FACTOR = 3.0          # MeshIndex: default cell / mean longest box side of the faces (measured: DESIGN.md §4.15)
MAX_MESH_REFS = 1 << 27         # MeshIndex: most (cell, face) references accepted by default (16 B each, and the sort's copy)
MAX_MESH_REFS_LIMIT = 1 << 40   # the kernels' cap (csrc/meshdist.hip MD_MAX_CAP)
RAY_MODES = ("first", "any", "count")    # cast_rays: the values of md_mode (csrc/meshray.hip)
MAX_ISECT_PAIRS = 1 << 26       # intersections: most reported pairs accepted by default (17 B each, and the sort's copy)
ISECT_KINDS = {"crossing": _lib.ISECT["CROSSING"], "coplanar": _lib.ISECT["COPLANAR"],
               "uncertain": _lib.ISECT["UNCERTAIN"]}       # the kind of a pair (csrc/meshintersect.hip)
WINDING_LEAF_FACTOR = 2.0       # winding: leaf edge of the octree / mean longest box side of the faces (measured: DESIGN.md §4.22)
WINDING_BETA = 2.0              # winding: a node farther than beta radii from the query is replaced by its expansion
WINDING_RAW, WINDING_REC = 40, 32    # doubles per node: raw moments, node record (csrc/meshwinding.hip WN_RAW, WN_REC)
INSIDE_METHODS = ("parity", "winding")
# contains_points: three fixed directions in general position (no component zero, no two equal in magnitude, pairwise far
# from parallel), so that a ray meets an edge or a vertex of an axis-aligned or regularly gridded mesh only by accident
INSIDE_DIRECTIONS = ((0.5370861555295747, 0.2915274230636872, 0.7915368220043530),
                     (-0.6812409104782753, 0.6469328946524311, 0.3425017306508174),
                     (0.3129804157290411, -0.8331402637850166, -0.4560219781334682))
KEEP = 1

PROTOCOLS = {
    "dtu": dict(downsample_density=0.2, patch_size=60.0, max_dist=20.0, visualize_threshold=10.0, thresholds=(1.0, 2.0),
                decimals=3),
    "deepfashion": dict(downsample_density=0.002, patch_size=60.0, max_dist=0.1, visualize_threshold=0.01,
                        thresholds=(0.001, 0.002), decimals=6),
}


# ---- argument checks -------------------------------------------------------------------------------------------------
def _device(*ts):
    """the device of the first GPU tensor among ts, else the current GPU"""
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda")


def _shape3(p, name):
    """p as a floating-point [N, 3] tensor (not moved); ValueError otherwise"""
    t = torch.as_tensor(p) if not isinstance(p, torch.Tensor) else p
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [N, 3] (got {tuple(t.shape)})")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point array (got {t.dtype})")
    return t


def _points(p, name, dev, finite=True):
    """-> contiguous float64 [N, 3] on dev"""
    t = _shape3(p, name).to(device=dev, dtype=torch.float64).contiguous()
    if finite and t.numel() and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} holds non-finite coordinates")
    return t


def _positive(v, name, allow_inf=False):
    v = float(v)
    if not (v > 0 and (allow_inf or math.isfinite(v))):
        raise ValueError(f"{name} must be a {'' if allow_inf else 'finite '}positive number (got {v})")
    return v


def _grid_size(lo, hi, cell):
    """(cell, grid) with every axis's cell count within the 21-bit key (the cell grows when it would not fit)"""
    ext = max(h - l for l, h in zip(lo, hi))
    cell = max(cell, ext / (AXIS_CELLS - 4))
    if not cell > 0:
        cell = 1.0
    grid = [min(int(math.floor((h - l) / cell)) + 2, AXIS_CELLS) for l, h in zip(lo, hi)]
    return cell, grid


# ---- mesh sampling ---------------------------------------------------------------------------------------------------
def sample_mesh(vertices, faces, density, *, max_points=MAX_POINTS):
    """the reference's mesh sampling (eval_dtu_python.py:225-258): every vertex, then for each triangle of non-zero area
    in triangle order the points (v1 c0 + v2 c1) + t0 of its (n1 + 1) x (n2 + 1) lattice with c0 + c1 < 1, all in float64
    with numpy's operation order.  vertices [V, 3] (NaN allowed: its triangles drop out, as in the reference; +-inf is
    refused), faces [F, 3] integer indices.  -> points [V + M, 3] float64 on the GPU.  Raises ValueError when the cloud
    would exceed max_points (a tiny density on a big mesh)."""
    density = _positive(density, "density")
    max_points = int(max_points)
    _shape3(vertices, "vertices")
    f = torch.as_tensor(faces) if not isinstance(faces, torch.Tensor) else faces
    if f.dim() != 2 or f.shape[1] != 3 or f.is_floating_point() or f.is_complex() or f.dtype == torch.bool:
        raise ValueError(f"faces must be an integer [F, 3] array (got {tuple(f.shape)}, {f.dtype})")
    dev = _device(vertices, faces)
    v = _points(vertices, "vertices", dev, finite=False)
    if bool(torch.isinf(v).any()):
        raise ValueError("vertices hold infinite coordinates")
    f = f.to(device=dev, dtype=torch.int64).contiguous()
    nv, nf = v.shape[0], f.shape[0]
    if nf and (int(f.min()) < 0 or int(f.max()) >= nv):
        raise ValueError(f"face index out of range [0, {nv})")
    if nv > max_points:
        raise ValueError(f"{nv} vertices exceed max_points={max_points}")
    if nf == 0:
        return v.clone()
    tri_n = torch.empty(nf, dtype=torch.int64, device=dev)
    d = _lib.PointCloud(verts=ptr(v), faces=ptr(f), tri_n=ptr(tri_n), n_verts=nv, n_faces=nf, cap=max_points - nv,
                        density=density)
    call("nudf_pc_tri_count", d)
    ends = torch.cumsum(tri_n, 0)
    m = int(ends[-1])
    if nv + m > max_points:
        raise ValueError(f"sampling at density {density} gives more than max_points={max_points} points: "
                         "raise the density or max_points")
    out = torch.empty((nv + m, 3), dtype=torch.float64, device=dev)
    out[:nv] = v
    off = ends - tri_n
    d.tri_off, d.out, d.n_out, d.out_base = ptr(off), ptr(out), nv + m, nv
    call("nudf_pc_tri_emit", d)
    return out


# ---- the cell index --------------------------------------------------------------------------------------------------
class _CellIndex:
    """points sorted by packed cell key (stable: by index inside a cell), the occupied-cell table and its hash"""

    def __init__(self, pts, cell, lo=None, hi=None):
        dev = pts.device
        if lo is None:
            lo, hi = pts.min(0).values.tolist(), pts.max(0).values.tolist()
        self.lo, self.hi = lo, hi
        self.cell, self.grid = _grid_size(lo, hi, cell)
        n = pts.shape[0]
        self.d = _lib.PointCloud(n=n, cell=self.cell)
        self.d.origin[:] = lo
        self.d.grid[:] = self.grid
        keys = self.keys_of(pts)
        skeys, order = torch.sort(keys, stable=True)
        self.keys, self.rank = skeys, order
        self.pts = pts[order].contiguous()
        ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
        self.cell_key, self.cell_count = ukeys.contiguous(), counts.contiguous()
        self.cell_start = (torch.cumsum(counts, 0) - counts).contiguous()
        nc = ukeys.numel()
        cap = 1 << max(1, (2 * nc - 1).bit_length())
        self.hash_key = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        self.hash_row = torch.empty(cap, dtype=torch.int64, device=dev)
        d = self.d
        d.pts, d.keys, d.rank = ptr(self.pts), ptr(self.keys), ptr(self.rank)
        d.cell_key, d.cell_start, d.cell_count, d.n_cells = ptr(self.cell_key), ptr(self.cell_start), ptr(counts), nc
        d.hash_key, d.hash_row, d.hash_cap = ptr(self.hash_key), ptr(self.hash_row), cap
        call("nudf_pc_cells", d)

    def keys_of(self, pts):
        keys = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
        k = _lib.PointCloud(pts=ptr(pts), n=pts.shape[0], cell=self.cell, keys=ptr(keys))
        k.origin[:] = self.lo
        call("nudf_pc_keys", k)
        return keys

    @property
    def n_cells(self):
        return self.cell_key.numel()


def _occupancy(pts, cell, lo, hi):
    """mean points per occupied cell of edge `cell` (and the cell actually used)"""
    idx = _CellIndex.__new__(_CellIndex)
    idx.lo = lo
    idx.cell, _ = _grid_size(lo, hi, cell)
    keys = idx.keys_of(pts)
    return pts.shape[0] / torch.unique(keys).numel(), idx.cell


def nearest_cell_size(ref, target=NEAREST_POINTS_PER_CELL):
    """cell edge of the nearest-neighbour index: `target` points per occupied cell on average.  Starts from the cube of the
    box holding n / target cells and rescales twice by sqrt(target / measured), the law of a surface-like cloud."""
    lo, hi = ref.min(0).values.tolist(), ref.max(0).values.tolist()
    ext = max(h - l for l, h in zip(lo, hi))
    n = ref.shape[0]
    if not ext > 0 or n <= target:
        return _grid_size(lo, hi, ext if ext > 0 else 1.0)[0]
    cell = ext / max(1.0, (n / target) ** (1.0 / 3.0))
    for _ in range(2):
        m, cell = _occupancy(ref, cell, lo, hi)
        cell *= math.sqrt(target / m)
    return _grid_size(lo, hi, cell)[0]


# ---- thinning --------------------------------------------------------------------------------------------------------
def thin(points, radius, _info=None):
    """the reference's radius down-sampling mask (eval_dtu_python.py:265-276) for points already in rank order: point i is
    kept iff no kept point of lower index lies within `radius` (distance <= radius, boundary included, d^2 compared with
    radius * radius as sklearn does).  -> keep [N] bool on the GPU.  (`_info`: a dict that receives the round count.)"""
    r = _positive(radius, "radius")
    _shape3(points, "points")
    dev = _device(points)
    p = _points(points, "points", dev)
    n = p.shape[0]
    if n == 0:
        if _info is not None:
            _info["rounds"] = 0
        return torch.zeros(0, dtype=torch.bool, device=dev)
    idx = _CellIndex(p, r * THIN_CELL_SLACK)
    state = torch.zeros(n, dtype=torch.uint8, device=dev)
    undecided = torch.zeros(1, dtype=torch.int32, device=dev)
    d = idx.d
    d.state, d.undecided, d.r2 = ptr(state), ptr(undecided), r * r
    rounds = 0
    while True:
        undecided.zero_()
        call("nudf_pc_thin_round", d)
        rounds += 1
        left = int(undecided.item())
        if left == 0:
            break
        if rounds > n:                     # each round decides the lowest-ranked undecided point: cannot happen
            raise RuntimeError(f"thinning did not finish in {n} rounds ({left} points undecided)")
    keep = torch.empty(n, dtype=torch.bool, device=dev)
    keep[idx.rank] = state == KEEP
    if _info is not None:
        _info["rounds"] = rounds
    return keep


def radius_downsample(points, radius, seed=0):
    """shuffle (a seeded permutation) then thin: the reference's data_down, in shuffled order.
    -> (points_down [K, 3] float64, info dict(perm [N] int64, keep [N] bool in shuffled order, rounds))"""
    _positive(radius, "radius")
    _shape3(points, "points")
    dev = _device(points)
    p = _points(points, "points", dev)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    perm = torch.randperm(p.shape[0], generator=g, device=dev)
    shuffled = p[perm]
    info = {}
    keep = thin(shuffled, radius, _info=info)
    info.update(perm=perm, keep=keep)
    return shuffled[keep], info


# ---- nearest neighbours ----------------------------------------------------------------------------------------------
def nearest(query, ref, bound=math.inf, *, cell=None, _events=None):
    """nearest point of `ref` for every point of `query` (sklearn kneighbors with n_neighbors=1): the float64 distance
    sqrt(((dx dx) + (dy dy)) + (dz dz)) and the lowest index of ref achieving it.  Distances beyond `bound` are reported as
    +inf with index -1 (they leave every metric of the protocols unchanged when bound >= max_dist and the thresholds).
    -> (dist [M] float64, idx [M] int64) on the GPU.  (`cell`: the index's cell edge, by default nearest_cell_size.)"""
    bound = _positive(bound, "bound", allow_inf=True)
    if _shape3(ref, "ref").shape[0] == 0:
        raise ValueError("the reference cloud is empty")
    _shape3(query, "query")
    dev = _device(query, ref)
    q = _points(query, "query", dev)
    r = _points(ref, "ref", dev)
    m = q.shape[0]
    dist = torch.empty(m, dtype=torch.float64, device=dev)
    idx = torch.empty(m, dtype=torch.int64, device=dev)
    if m == 0:
        return dist, idx
    index = _CellIndex(r, nearest_cell_size(r) if cell is None else _positive(cell, "cell"))
    qkeys = index.keys_of(q)
    qorder = torch.sort(qkeys, stable=True).indices
    qs = q[qorder].contiguous()
    d = index.d
    d.query, d.query_idx, d.n_query, d.bound = ptr(qs), ptr(qorder), m, bound
    d.box_bound2 = (bound * (1.0 + 1e-9)) ** 2 if math.isfinite(bound) else math.inf
    d.box_lo[:], d.box_hi[:] = index.lo, index.hi
    d.dist, d.idx = ptr(dist), ptr(idx)
    if _events is not None:
        _events["cell"] = index.cell
        _events["cells"] = index.n_cells
    call("nudf_pc_nearest", d)
    return dist, idx


# ---- exact point-to-mesh distance ------------------------------------------------------------------------------------
class RayHits(NamedTuple):
    """t [N] float64 in units of the direction (+inf on a miss); face [N] int64 (-1 on a miss); bary [N, 3] float64: the
    weights of the hit at the corners of `face`, in the face's corner order (NaN on a miss)"""
    t: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor


class Closest(NamedTuple):
    """dist [M] float64; face [M] int64 (-1 beyond bound); point [M, 3] float64: the closest point of the mesh; bary
    [M, 3] float64: its weights at the corners of `face`, in the face's corner order (NaN beyond bound, as point)"""
    dist: torch.Tensor
    face: torch.Tensor
    point: torch.Tensor
    bary: torch.Tensor


class Intersections(NamedTuple):
    """pairs [P, 2] int64 sorted by (a, b): in a self run two faces of the mesh, a < b; against another mesh (face of that
    mesh, face of the indexed mesh).  kind [P] int8, a value of ISECT_KINDS.  face_mask [F] bool: the faces of the indexed
    mesh that are in a pair."""
    pairs: torch.Tensor
    kind: torch.Tensor
    face_mask: torch.Tensor


class MeshIntersections(NamedTuple):
    """pairs [P, 2] int64 (face of a, face of b) sorted; kind [P] int8; mask_a [Fa] bool, mask_b [Fb] bool: the faces of
    either mesh that are in a pair"""
    pairs: torch.Tensor
    kind: torch.Tensor
    mask_a: torch.Tensor
    mask_b: torch.Tensor


def _check_face_array(faces):
    f = torch.as_tensor(faces) if not isinstance(faces, torch.Tensor) else faces
    if f.dim() != 2 or f.shape[1] != 3 or f.is_floating_point() or f.is_complex() or f.dtype == torch.bool:
        raise ValueError(f"faces must be an integer [F, 3] array (got {tuple(f.shape)}, {f.dtype})")
    return f


def _stage(events, name):
    """closes the open stage of the event dict and opens `name` (None: closes only); nothing without a dict"""
    if events is None:
        return
    last = events.get("_open")
    if last is not None:
        events[last][1].record()
    events["_open"] = name
    if name is not None:
        events[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        events[name][0].record()
    else:
        del events["_open"]


class MeshIndex:
    """the faces of a mesh binned into a uniform grid for closest_on_mesh and cast_rays: every face is listed in each cell
    its axis-aligned box touches (csrc/meshdist.hip tribin_count / tribin_emit, a torch int64 scan between them), the
    (cell, face) references sorted by cell (stable: ascending face inside a cell), the occupied-cell table and its hash
    (nudf_pc_cells).  Build once, query many times.

    vertices [V, 3] (NaN allowed: its faces are absent; +-inf is refused), faces [F, 3] integer indices.  `cell`: the
    grid's edge; by default MESH_CELL_FACTOR times the mean longest box side of the faces -- a property of the mesh, not
    of the queries.  Either way the cell doubles until the reference count fits `max_refs`.  ValueError: no face, no
    usable face (every face has a NaN vertex), an index out of range, infinite vertices, more than max_refs faces.
    (`_events`: a dict that receives a pair of events per stage: count, scan, emit, sort, cells.)"""

    def __init__(self, vertices, faces, cell=None, max_refs=MAX_MESH_REFS, _events=None):
        _shape3(vertices, "vertices")
        f = _check_face_array(faces)
        dev = _device(vertices, faces)
        v = _points(vertices, "vertices", dev, finite=False)
        if bool(torch.isinf(v).any()):
            raise ValueError("vertices hold infinite coordinates")
        f = f.to(device=dev, dtype=torch.int64).contiguous()
        nv, nf = v.shape[0], f.shape[0]
        if nf == 0:
            raise ValueError("the mesh has no faces")
        if int(f.min()) < 0 or int(f.max()) >= nv:
            raise ValueError(f"face index out of range [0, {nv})")
        max_refs = int(max_refs)
        if not 0 < max_refs <= MAX_MESH_REFS_LIMIT:
            raise ValueError(f"max_refs must lie in [1, 2^40] (got {max_refs})")
        corners = v[f]                                                          # [F, 3, 3]
        usable = torch.isfinite(corners).all(2).all(1)
        n_usable = int(usable.sum())
        if n_usable == 0:
            raise ValueError("the mesh has no usable face: every face has a non-finite vertex")
        if n_usable > max_refs:
            raise ValueError(f"{n_usable} faces exceed max_refs={max_refs} even with one cell per axis")
        corners = corners[usable]
        lo, hi = corners.amin((0, 1)).tolist(), corners.amax((0, 1)).tolist()
        ext = max(h - l for l, h in zip(lo, hi))
        if cell is None:
            cell = MESH_CELL_FACTOR * float((corners.amax(1) - corners.amin(1)).amax(1).mean())
            if not cell > 0:
                cell = ext if ext > 0 else 1.0
        else:
            cell = _positive(cell, "cell")
        del corners
        self.vertices, self.faces, self.lo, self.hi, self.n_usable = v, f, lo, hi, n_usable
        ref_n = torch.empty(nf, dtype=torch.int64, device=dev)
        d = _lib.PointCloud(verts=ptr(v), faces=ptr(f), n_verts=nv, n_faces=nf, cap=max_refs, md_ref_n=ptr(ref_n))
        d.origin[:], d.box_lo[:], d.box_hi[:] = lo, lo, hi
        while True:
            self.cell, self.grid = _grid_size(lo, hi, cell)
            d.cell = self.cell
            d.grid[:] = self.grid
            _stage(_events, "count")
            call("nudf_pc_tribin_count", d)
            _stage(_events, "scan")
            ends = torch.cumsum(ref_n, 0)
            n_refs = int(ends[-1])
            if n_refs <= max_refs:
                break
            if self.cell > ext:                  # one cell holds the mesh: refs = faces <= max_refs, cannot happen
                raise ValueError(f"{n_refs} references exceed max_refs={max_refs} even with one cell per axis")
            cell = self.cell * 2.0
        _stage(_events, "emit")
        off = (ends - ref_n).contiguous()
        ref_key = torch.empty(n_refs, dtype=torch.int64, device=dev)
        ref_face = torch.empty(n_refs, dtype=torch.int64, device=dev)
        d.md_ref_off, d.md_ref_key, d.md_ref_face, d.md_n_refs = ptr(off), ptr(ref_key), ptr(ref_face), n_refs
        call("nudf_pc_tribin_emit", d)
        _stage(_events, "sort")
        skeys, order = torch.sort(ref_key, stable=True)
        self.cell_face = ref_face[order].contiguous()
        _stage(_events, "cells")
        ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
        self.cell_key, self.cell_count = ukeys.contiguous(), counts.contiguous()
        self.cell_start = (torch.cumsum(counts, 0) - counts).contiguous()
        nc = ukeys.numel()
        cap = 1 << max(1, (2 * nc - 1).bit_length())
        self.hash_key = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        self.hash_row = torch.empty(cap, dtype=torch.int64, device=dev)
        d.cell_key, d.cell_start, d.cell_count, d.n_cells = ptr(self.cell_key), ptr(self.cell_start), ptr(self.cell_count), nc
        d.hash_key, d.hash_row, d.hash_cap = ptr(self.hash_key), ptr(self.hash_row), cap
        call("nudf_pc_cells", d)
        _stage(_events, None)
        d.md_cell_face = ptr(self.cell_face)
        d.md_ref_n = d.md_ref_off = d.md_ref_key = d.md_ref_face = None        # the scratch of the build is released
        self.d, self.n_refs, self.n_cells = d, n_refs, nc
        self._winding_tree = None

    def keys_of(self, pts):
        keys = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
        k = _lib.PointCloud(pts=ptr(pts), n=pts.shape[0], cell=self.cell, keys=ptr(keys))
        k.origin[:] = self.lo
        call("nudf_pc_keys", k)
        return keys

    def closest(self, query, bound=math.inf, _events=None):
        """closest_on_mesh(query, index=self, bound=bound)  (`_events`: receives the stages query_sort and closest)"""
        bound = _positive(bound, "bound", allow_inf=True)
        _shape3(query, "query")
        dev = self.vertices.device
        q = _points(query, "query", dev)
        m = q.shape[0]
        out = Closest(torch.empty(m, dtype=torch.float64, device=dev), torch.empty(m, dtype=torch.int64, device=dev),
                      torch.empty((m, 3), dtype=torch.float64, device=dev),
                      torch.empty((m, 3), dtype=torch.float64, device=dev))
        if m == 0:
            return out
        _stage(_events, "query_sort")
        qorder = torch.sort(self.keys_of(q), stable=True).indices
        qs = q[qorder].contiguous()
        _stage(_events, "closest")
        d = self.d
        d.query, d.query_idx, d.n_query, d.bound = ptr(qs), ptr(qorder), m, bound
        d.box_bound2 = (bound * (1.0 + 1e-9)) ** 2 if math.isfinite(bound) else math.inf
        d.dist, d.idx, d.md_point, d.md_bary = ptr(out.dist), ptr(out.face), ptr(out.point), ptr(out.bary)
        call("nudf_pc_closest", d)
        _stage(_events, None)
        d.query = d.query_idx = d.dist = d.idx = d.md_point = d.md_bary = None
        return out

    def cast(self, origins, directions, t_min=0.0, t_max=math.inf, mode="first", _events=None):
        """rays against the mesh of this index (cast_rays with index=self): `mode` "first" -> RayHits(t, face, bary), "any" ->
        [N] bool, "count" -> [N] int64, in the caller's order.  t_min / t_max: numbers, or [N] tensors for a window per ray.
        (`_events`: receives the stages ray_sort and cast.)"""
        if mode not in RAY_MODES:
            raise ValueError(f"mode must be one of {RAY_MODES} (got {mode!r})")
        _shape3(origins, "origins"), _shape3(directions, "directions")
        dev = self.vertices.device
        o, d = _rays(origins, directions, dev)
        n = o.shape[0]
        t_min, t_max, window = _window(t_min, t_max, n, dev)
        if mode == "first":
            out = RayHits(torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                          torch.empty((n, 3), dtype=torch.float64, device=dev))
            count = None
        else:
            out, count = None, torch.empty(n, dtype=torch.int64, device=dev)
        if n:
            _stage(_events, "ray_sort")
            # coherence only: the cell in which the ray enters the grid's box (the origin's when it starts inside; for a
            # ray that misses the box, a point of its line clamped into it); the order changes no result
            lo = torch.tensor(self.lo, dtype=torch.float64, device=dev)
            hi = torch.tensor(self.hi, dtype=torch.float64, device=dev)
            inv = 1.0 / torch.where(d == 0, torch.full_like(d, 1e-300), d)
            ta, tb = (lo - o) * inv, (hi - o) * inv
            enter = torch.minimum(ta, tb).amax(1).clamp_min(0.0)
            entry = torch.nan_to_num(o + enter[:, None] * d, nan=0.0, posinf=0.0, neginf=0.0)
            entry = torch.maximum(torch.minimum(entry, hi), lo).contiguous()
            order = torch.sort(self.keys_of(entry), stable=True).indices
            so, sd = o[order].contiguous(), d[order].contiguous()
            sw = None if window is None else window[order].contiguous()
            _stage(_events, "cast")
            r = self.d
            r.md_ray_o, r.md_ray_d, r.query_idx, r.n_query = ptr(so), ptr(sd), ptr(order), n
            r.md_t_min, r.md_t_max, r.md_ray_window, r.md_mode = t_min, t_max, ptr(sw), RAY_MODES.index(mode)
            if mode == "first":
                r.dist, r.idx, r.md_bary = ptr(out.t), ptr(out.face), ptr(out.bary)
            else:
                r.md_count = ptr(count)
            call("nudf_pc_raycast", r)
            _stage(_events, None)
            r.md_ray_o = r.md_ray_d = r.query_idx = r.md_ray_window = r.dist = r.idx = r.md_bary = r.md_count = None
        if mode == "first":
            return out
        return count != 0 if mode == "any" else count

    def intersections(self, other=None, max_pairs=MAX_ISECT_PAIRS, _events=None):
        """the faces of this mesh that pass through each other, or with `other` ((vertices, faces) or a MeshIndex) the
        faces of that mesh against the faces of this one -> Intersections (self_intersections, mesh_intersections;
        csrc/meshintersect.hip isect_count / isect_emit, a torch int64 scan between them and one stable sort of the pairs
        after them).  More than `max_pairs` reported pairs raise ValueError after the count pass.
        (`_events`: receives the stages count, scan, emit, sort.)"""
        try:
            ok = int(max_pairs) == max_pairs and int(max_pairs) >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"max_pairs must be a non-negative integer (got {max_pairs!r})")
        max_pairs = int(max_pairs)
        dev, nf = self.vertices.device, self.faces.shape[0]
        if other is None:
            corners, nq = None, nf
        else:
            ov, of = _mesh_arrays(other, "other", dev)
            corners, nq = ov[of].contiguous(), of.shape[0]
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        mask = torch.zeros(nf, dtype=torch.bool, device=dev)
        if nq == 0:
            return Intersections(empty.reshape(0, 2), empty.to(torch.int8), mask)
        ref_n = torch.empty(nq, dtype=torch.int64, device=dev)
        d, cap = self.d, self.d.cap
        d.query, d.n_query, d.md_mode, d.md_ref_n, d.cap = ptr(corners), nq, 0 if other is None else 1, ptr(ref_n), max_pairs
        try:
            _stage(_events, "count")
            call("nudf_pc_isect_count", d)
            _stage(_events, "scan")
            ends = torch.cumsum(ref_n, 0)
            total = int(ends[-1])
            if total > max_pairs:
                raise ValueError(f"{total} intersecting pairs exceed max_pairs={max_pairs}")
            _stage(_events, "emit")
            off = (ends - ref_n).contiguous()
            a = torch.empty(total, dtype=torch.int64, device=dev)
            b = torch.empty(total, dtype=torch.int64, device=dev)
            kind = torch.empty(total, dtype=torch.uint8, device=dev)
            d.md_ref_off, d.md_ref_key, d.md_ref_face, d.state, d.cap = ptr(off), ptr(a), ptr(b), ptr(kind), total
            call("nudf_pc_isect_emit", d)
            _stage(_events, "sort")
            order = torch.sort(a * nf + b, stable=True).indices
            pairs, kind = torch.stack([a[order], b[order]], 1), kind[order].to(torch.int8)
        finally:
            _stage(_events, None)
            d.query = d.md_ref_n = d.md_ref_off = d.md_ref_key = d.md_ref_face = d.state = None
            d.n_query, d.md_mode, d.cap = 0, 0, cap
        mask[pairs[:, 1]] = True
        if other is None:
            mask[pairs[:, 0]] = True
        return Intersections(pairs, kind, mask)


    def winding(self, points, beta=WINDING_BETA, _events=None, _counts=False):
        """winding_number(points, self, beta) -> [M] float64 in the caller's order.  The octree is built on the first call
        and kept on the index.  (`_events`: receives the stages of the build -- keys, sort, levels, moments -- when this
        call builds the tree, and query_sort and winding; `_counts`: -> (w, the faces evaluated exactly [M] int64, the
        nodes replaced by their expansion [M] int64).)"""
        beta = float(beta)
        if not beta >= 1.0:
            raise ValueError(f"beta must be >= 1 (got {beta})")
        _shape3(points, "points")
        dev = self.vertices.device
        q = _points(points, "points", dev)
        m = q.shape[0]
        w = torch.zeros(m, dtype=torch.float64, device=dev)
        exact = torch.zeros(m, dtype=torch.int64, device=dev) if _counts else None
        far = torch.zeros(m, dtype=torch.int64, device=dev) if _counts else None
        if m:
            if self._winding_tree is None:
                self._winding_tree = _WindingTree(self, _events)
            tree = self._winding_tree
            if tree.n_nodes:                               # no face with an area: w = 0 everywhere
                _stage(_events, "query_sort")              # coherence only: the order changes no result
                qorder = torch.sort(tree.keys_of(q, 1), stable=True).indices
                qs = q[qorder].contiguous()
                _stage(_events, "winding")
                d = tree.d
                d.query, d.query_idx, d.n_query, d.r2 = ptr(qs), ptr(qorder), m, beta * beta
                d.dist, d.md_count, d.idx = ptr(w), ptr(exact), ptr(far)
                try:
                    call("nudf_pc_winding", d)
                finally:
                    _stage(_events, None)
                    d.query = d.query_idx = d.dist = d.md_count = d.idx = None
                    d.n_query = 0
        return (w, exact, far) if _counts else w


class _WindingTree:
    """the linear octree of MeshIndex.winding (restated in tests/meshwinding_ref.py): the usable faces
    sorted by the Morton key of their centroid's leaf cell, a node per distinct key >> 3 l on every level l up to the first
    with one node, the nodes in preorder with a skip index, and a record of 32 doubles per node (csrc/meshwinding.hip
    wn_faces / wn_nodes; the sorts, the level boundaries and the skip index are torch's)"""

    def __init__(self, index, _events=None):
        v, f = index.vertices, index.faces
        dev = v.device
        corners = v[f]
        corners = corners[torch.isfinite(corners).all(2).all(1)]
        leaf = WINDING_LEAF_FACTOR * float((corners.amax(1) - corners.amin(1)).amax(1).mean())
        del corners
        lo, hi = index.lo, index.hi
        if not leaf > 0:
            ext = max(h - l for l, h in zip(lo, hi))
            leaf = ext if ext > 0 else 1.0
        while True:                                        # the leaf edge doubles until the grid fits the key
            grid = [int(math.floor((h - l) / leaf)) + 1 for l, h in zip(lo, hi)]
            if max(grid) <= AXIS_CELLS:
                break
            leaf *= 2.0
        self.leaf, self.grid, self.device = leaf, grid, dev
        nv, nf = v.shape[0], f.shape[0]
        d = _lib.PointCloud(verts=ptr(v), faces=ptr(f), n_verts=nv, n_faces=nf, cell=leaf)
        d.origin[:], d.grid[:] = lo, grid
        self.d = d
        _stage(_events, "keys")
        keys = self.keys_of(None, 0)
        _stage(_events, "sort")
        skeys, order = torch.sort(keys, stable=True)
        present = skeys >= 0
        skeys, order = skeys[present], order[present].contiguous()
        n = skeys.numel()
        self.faces, self.n_nodes = order, 0
        if n == 0:
            _stage(_events, None)
            return
        _stage(_events, "levels")
        first, level = [], []
        for ell in range(22):
            ids = skeys >> (3 * ell)
            new = torch.ones(n, dtype=torch.bool, device=dev)
            new[1:] = ids[1:] != ids[:-1]
            start = torch.nonzero(new).reshape(-1)
            first.append(start)
            level.append(torch.full_like(start, ell))
            if start.numel() == 1:
                break
        ends = [torch.cat([s[1:], s.new_tensor([n])]) for s in first]
        first, end, level = torch.cat(first), torch.cat(ends), torch.cat(level)
        pre = torch.sort(first * 32 + (31 - level), stable=True).indices        # preorder: first face, level descending
        first, end, level = first[pre].contiguous(), end[pre].contiguous(), level[pre]
        self.first, self.count, self.level = first, (end - first).contiguous(), level
        self.skip = torch.searchsorted(first, end).contiguous()
        nn = first.numel()
        self.raw = torch.empty((nn, WINDING_RAW), dtype=torch.float64, device=dev)
        self.rec = torch.empty((nn, WINDING_REC), dtype=torch.float64, device=dev)
        d.md_cell_face, d.md_n_refs, d.n = ptr(order), n, nn
        d.rank, d.cell_start, d.cell_count = ptr(self.skip), ptr(first), ptr(self.count)
        d.out, d.md_point, d.pts = ptr(self.raw), ptr(self.rec), ptr(self.rec)
        _stage(_events, "moments")
        for ell in range(int(level.max()) + 1):            # bottom-up: a parent reads what the level below wrote
            nodes = torch.nonzero(level == ell).reshape(-1).contiguous()
            d.query_idx, d.n_query = ptr(nodes), nodes.numel()
            call("nudf_pc_wn_nodes", d)
        _stage(_events, None)
        d.query_idx, d.n_query, d.out, d.md_point = None, 0, None, None
        self.raw = None                                    # the scratch of the build is released
        self.n_nodes = nn

    def keys_of(self, pts, mode):
        """the Morton keys of the faces' leaf cells (mode 0; -1: absent) or of the cells of pts (mode 1)"""
        n = self.d.n_faces if mode == 0 else pts.shape[0]
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        k = _lib.PointCloud(verts=self.d.verts, faces=self.d.faces, n_verts=self.d.n_verts, n_faces=self.d.n_faces,
                            cell=self.leaf, query=None if mode == 0 else ptr(pts), n_query=n, md_mode=mode, keys=ptr(keys))
        k.origin[:], k.grid[:] = list(self.d.origin), self.grid
        call("nudf_pc_wn_faces", k)
        return keys


def winding_number(points, mesh, beta=WINDING_BETA):
    """[M] float64: the generalised winding number of `mesh` ((vertices, faces) or a MeshIndex) at `points` [M, 3]
    (Jacobson et al. 2013; the tree of Barill et al. 2018, what libigl's fast_winding_number answers on the CPU), in the
    caller's order: w(q) = 1 / (4 pi) times the sum over the faces of the signed solid angle under which q sees them.  1
    inside and 0 outside a closed mesh that is wound outward (-1 inside one wound inward); where faces are missing it
    falls off smoothly instead of flipping, and across an open sheet it jumps by one, from about +1/2 on the side the
    normals point away from to about -1/2 on the other, fading to 0 far from the sheet.  The value follows the faces'
    winding: on a mesh whose faces disagree the contributions cancel, so run meshclean.orient_faces first.

    A node of the octree farther than `beta` of its radii from the query (d^2 > beta^2 r^2) is replaced by its expansion
    to second order about its area-weighted centre; nearer leaves are summed exactly (van Oosterom and Strackee; a query
    in a face's plane gets 0 from that face).  beta=inf is the exact sum over all faces.  Measured errors: DESIGN.md
    §4.22 (at most 3e-3 at beta 2, 3e-4 at beta 3 on the test meshes).  Float64 without contraction; the tree, the moments and every decision
    of the walk equal tests/meshwinding_ref.py, the values up to atan2.  A face with a non-finite vertex or no area is
    absent.  Non-finite points raise ValueError; empty input gives empty output."""
    return _as_index(mesh, "mesh").winding(points, beta)


def closest_on_mesh(query, vertices=None, faces=None, bound=math.inf, *, index=None, cell=None):
    """the closest point of a triangle mesh for every point of `query` [M, 3], exactly (what
    trimesh.proximity.closest_point answers on the CPU) -> Closest(dist, face, point, bary) on the GPU, in the caller's
    order.  Per face the candidates are the interior (the foot of the perpendicular, when it falls strictly inside) and
    the three edges, each evaluated from its lower vertex index to its higher, end points taken exactly: a query that is
    a mesh vertex gets 0.0, two faces sharing an edge agree to the bit, the winding changes nothing.  Across faces the
    smallest (squared distance, face index) wins, so the result depends neither on the cell size nor on the order of
    traversal; it equals tests/meshdist_ref.py bit for bit.  Degenerate faces count as their edges; a face with a NaN
    vertex is absent.  Rows beyond `bound` are +inf / -1 / NaN / NaN.  Non-finite queries raise ValueError; an empty
    query gives empty outputs.  Pass either (vertices, faces[, cell]) or a MeshIndex built from them as `index`."""
    if index is None:
        if vertices is None or faces is None:
            raise ValueError("closest_on_mesh needs (vertices, faces) or index=MeshIndex(...)")
        _positive(bound, "bound", allow_inf=True)
        _shape3(query, "query")
        index = MeshIndex(vertices, faces, cell=cell)
    elif vertices is not None or faces is not None or cell is not None:
        raise ValueError("pass either (vertices, faces[, cell]) or index, not both")
    elif not isinstance(index, MeshIndex):
        raise ValueError("index must be a MeshIndex")
    return index.closest(query, bound)


# ---- rays against the mesh -------------------------------------------------------------------------------------------
def _rays(origins, directions, dev):
    o, d = _points(origins, "origins", dev), _points(directions, "directions", dev)
    if o.shape != d.shape:
        raise ValueError(f"origins and directions differ in shape ({tuple(o.shape)}, {tuple(d.shape)})")
    if d.numel() and not bool((d != 0).any(1).all()):
        raise ValueError("directions hold a zero vector")
    return o, d


def _window(t_min, t_max, n, dev):
    """(t_min, t_max, None) for two numbers, (0.0, inf, [n, 2] float64) when either is given per ray"""
    if not isinstance(t_min, torch.Tensor) and not isinstance(t_max, torch.Tensor):
        t_min, t_max = float(t_min), float(t_max)
        if math.isnan(t_min) or not t_max >= t_min:
            raise ValueError(f"the window needs t_min <= t_max (got {t_min}, {t_max})")
        return t_min, t_max, None
    w = torch.empty((n, 2), dtype=torch.float64, device=dev)
    for k, t in enumerate((t_min, t_max)):
        t = torch.as_tensor(t, dtype=torch.float64, device=dev)
        if t.dim() > 1 or (t.dim() == 1 and t.shape[0] != n):
            raise ValueError(f"a per-ray window must be [N] (got {tuple(t.shape)} for {n} rays)")
        w[:, k] = t
    if n and not bool((w[:, 1] >= w[:, 0]).all()):
        raise ValueError("the window needs t_min <= t_max on every ray (and no NaN)")
    return 0.0, math.inf, w


def cast_rays(origins, directions, vertices=None, faces=None, *, index=None, cell=None, t_min=0.0, t_max=math.inf,
              mode="first"):
    """rays origins [N, 3] + t directions [N, 3] against a triangle mesh, exactly (what trimesh.ray answers on the CPU:
    intersects_first / intersects_any / the length of intersects_location), on the GPU, in the caller's order.  `t` is in
    units of the direction, which need not be a unit vector; a hit needs t_min <= t <= t_max (numbers, or [N] tensors for
    a window per ray).

        mode="first"  -> RayHits(t, face, bary): the smallest (t, face index); a miss is +inf / -1 / NaN.  Inclusive at
                         edges and vertices: a ray through a shared edge or a vertex of a sheet never leaks through.
        mode="any"    -> [N] bool: some face is hit in the window (the same inclusive rule, early exit).
        mode="count"  -> [N] int64: the faces crossed in the window.  An edge function that is exactly zero counts as
                         positive in the edge's direction from its lower vertex index to its higher, so a crossing through
                         the interior of an edge that two faces share counts once, whatever their windings.  A ray
                         through a vertex gets a deterministic count that is not guaranteed to be one crossing.

    Per face the test is Woop-Benthin-Wald's (axes permuted so that the largest |d| is z, sheared, each edge function
    evaluated once from the lower vertex index to the higher) in float64 without contraction: it equals
    tests/meshray_ref.py bit for bit, and the winding and the corner a face starts at change no bit of t.  The walk
    through the index is conservative, so the result depends neither on the cell size nor on the order of traversal.  A
    face with a NaN vertex or a zero determinant is absent.  Non-finite origins and zero or non-finite directions raise
    ValueError; empty input gives empty output.  Pass either (vertices, faces[, cell]) or a MeshIndex as `index`."""
    if index is None:
        if vertices is None or faces is None:
            raise ValueError("cast_rays needs (vertices, faces) or index=MeshIndex(...)")
        if mode not in RAY_MODES:
            raise ValueError(f"mode must be one of {RAY_MODES} (got {mode!r})")
        _shape3(origins, "origins"), _shape3(directions, "directions")
        index = MeshIndex(vertices, faces, cell=cell)
    elif vertices is not None or faces is not None or cell is not None:
        raise ValueError("pass either (vertices, faces[, cell]) or index, not both")
    elif not isinstance(index, MeshIndex):
        raise ValueError("index must be a MeshIndex")
    return index.cast(origins, directions, t_min, t_max, mode)


def _inside_method(method):
    if method not in INSIDE_METHODS:
        raise ValueError(f"method must be one of {INSIDE_METHODS} (got {method!r})")
    return method


def contains_points(points, mesh, method="parity"):
    """[M] bool: which of `points` [M, 3] lie inside the closed mesh `mesh` ((vertices, faces) or a MeshIndex; what
    trimesh.Trimesh.contains answers): the parity of the faces crossed (cast_rays mode="count") along each of the three
    fixed generic directions INSIDE_DIRECTIONS, the majority of the three.  Meant for closed meshes (the zero set of an
    SDF network, extract_iso_mesh), where a generic ray from an inside point crosses the surface an odd number of times;
    the vote guards against a ray that happens to pass through a vertex.  An open mesh has no inside: the answer is
    still the majority parity, i.e. whether most of the three rays cross the sheet an odd number of times -- behind a
    single open sheet as seen along those directions, not enclosed by it.

    method="winding" answers |w| > 0.5 with w = winding_number(points, mesh) instead: right for a closed surface with
    holes, where a ray can leave through a hole; the absolute value makes a mesh that is wound inward as a whole work.
    The winding number follows the faces' winding, so run meshclean.orient_faces first on a mesh whose faces disagree.
    On an open sheet w runs from +1/2 to -1/2 across the sheet and |w| reaches 1/2 only on the sheet itself: nothing is
    inside, unless the sheet curls around the point far enough to cover more than half of its sky."""
    if _inside_method(method) == "winding":
        return _as_index(mesh, "mesh").winding(points).abs() > 0.5
    index = _as_index(mesh, "mesh")
    _shape3(points, "points")
    p = _points(points, "points", index.vertices.device)
    votes = torch.zeros(p.shape[0], dtype=torch.int64, device=p.device)
    for dk in INSIDE_DIRECTIONS:
        d = torch.tensor(dk, dtype=torch.float64, device=p.device).expand(p.shape[0], 3)
        votes += index.cast(p, d, mode="count") & 1
    return 2 * votes > len(INSIDE_DIRECTIONS)


def signed_distance(points, mesh, bound=math.inf, method="parity"):
    """[M] float64: closest_on_mesh's distance from `points` to `mesh` ((vertices, faces) or a MeshIndex), negative
    where contains_points says inside -- the magnitude is that distance bit for bit, +inf beyond `bound` with its sign
    kept.  For closed meshes; see contains_points for what the sign means on an open one.  `method`: contains_points'
    "parity" or "winding"; the winding number follows the faces' winding (run meshclean.orient_faces first), it keeps
    the sign right next to a hole, and across an open sheet, where it jumps from +1/2 to -1/2, no point counts as
    inside."""
    _inside_method(method)
    index = _as_index(mesh, "mesh")
    dist = index.closest(points, bound).dist
    return torch.where(contains_points(points, index, method), -dist, dist)


def _as_index(m, name):
    if isinstance(m, MeshIndex):
        return m
    if not isinstance(m, (tuple, list)) or len(m) != 2:
        raise ValueError(f"{name} must be (vertices, faces) or a MeshIndex")
    return MeshIndex(m[0], m[1])


def _mesh_arrays(m, name, dev):
    """(vertices float64 [V, 3], faces int64 [F, 3]) on dev of a MeshIndex or a (vertices, faces) pair; ValueError for an
    index out of range"""
    if isinstance(m, MeshIndex):
        return m.vertices.to(dev), m.faces.to(dev)
    if not isinstance(m, (tuple, list)) or len(m) != 2:
        raise ValueError(f"{name} must be (vertices, faces) or a MeshIndex")
    _shape3(m[0], f"{name} vertices")
    f = _check_face_array(m[1]).to(device=dev, dtype=torch.int64).contiguous()
    v = _points(m[0], f"{name} vertices", dev, finite=False)
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError(f"{name}: face index out of range [0, {v.shape[0]})")
    return v, f


# ---- intersecting faces --------------------------------------------------------------------------------------------------
def self_intersections(vertices=None, faces=None, *, index=None, cell=None, max_pairs=MAX_ISECT_PAIRS):
    """the pairs of faces of a mesh that pass through each other (MeshLab's "select self intersecting faces", libigl's
    and pymeshfix's test on the CPU) -> Intersections(pairs [P, 2] with a < b, kind, face_mask) on the GPU.

    Every decision is the sign of an orient3d or orient2d of input coordinates, in Shewchuk's operation order with his
    stage-A error bound: a certified sign is the exact sign, anything else is uncertain.  Kinds (ISECT_KINDS):
    "crossing": the faces share a point in exact arithmetic (Guigue and Devillers' interval test; for faces with one
    common vertex, the edge opposite to it in one face pierces the other); "coplanar": the faces lie in one plane as far
    as float64 can tell and no edge separates them, or two faces over a common edge are folded onto each other;
    "uncertain": some sign could not be certified and the six edges, each against the other face, do not decide either
    -- the faces touch or come closer than float64 resolves.  A pair that
    is not reported is disjoint in exact arithmetic apart from its shared vertices (its shared edge); faces with the same
    three vertices are not reported (the edge table sees them).  The kind is a function of the ordered pair and of the
    corner order of its faces: certification, not the exact answer, can differ between the two orders of a nearly
    degenerate pair.  The pairs and kinds equal tests/meshintersect_ref.py bit for bit and do not depend on the cell
    size.  A face with a NaN vertex is absent.  Pass either (vertices, faces[, cell]) or a MeshIndex as `index`."""
    if index is None:
        if vertices is None or faces is None:
            raise ValueError("self_intersections needs (vertices, faces) or index=MeshIndex(...)")
        index = MeshIndex(vertices, faces, cell=cell)
    elif vertices is not None or faces is not None or cell is not None:
        raise ValueError("pass either (vertices, faces[, cell]) or index, not both")
    elif not isinstance(index, MeshIndex):
        raise ValueError("index must be a MeshIndex")
    return index.intersections(max_pairs=max_pairs)


def mesh_intersections(a, b, max_pairs=MAX_ISECT_PAIRS):
    """the faces of mesh `a` that pass through faces of mesh `b`, each (vertices, faces) or a MeshIndex ->
    MeshIntersections(pairs (face of a, face of b), kind, mask_a, mask_b); the rule of self_intersections for faces
    without a common vertex.  The mesh with more faces is indexed (b on a tie), unless one of them comes as a MeshIndex
    already; the triangles of the other are the queries."""
    if isinstance(a, MeshIndex) and not isinstance(b, MeshIndex):
        index_a = True
    elif isinstance(b, MeshIndex):
        index_a = False
    else:
        for m, name in ((a, "a"), (b, "b")):
            if not isinstance(m, (tuple, list)) or len(m) != 2:
                raise ValueError(f"{name} must be (vertices, faces) or a MeshIndex")
        index_a = _check_face_array(a[1]).shape[0] > _check_face_array(b[1]).shape[0]
    if index_a:
        ia = _as_index(a, "a")
        r = ia.intersections(b, max_pairs)                       # (face of b, face of a)
        nb = _mesh_arrays(b, "b", ia.vertices.device)[1].shape[0]
        order = torch.sort(r.pairs[:, 1] * max(nb, 1) + r.pairs[:, 0], stable=True).indices
        pairs, kind, mask_a = r.pairs[order].flip(1).contiguous(), r.kind[order], r.face_mask
        mask_b = torch.zeros(nb, dtype=torch.bool, device=pairs.device)
        mask_b[pairs[:, 1]] = True
        return MeshIntersections(pairs, kind, mask_a, mask_b)
    ib = _as_index(b, "b")
    r = ib.intersections(a, max_pairs)
    na = _mesh_arrays(a, "a", ib.vertices.device)[1].shape[0]
    mask_a = torch.zeros(na, dtype=torch.bool, device=r.pairs.device)
    mask_a[r.pairs[:, 0]] = True
    return MeshIntersections(r.pairs, r.kind, mask_a, r.face_mask)


def _one_sided(src, dst, density, bound):
    """from the finite vertices of src (with density: sample_mesh's cloud, which begins with them) to the surface of dst"""
    pts = src.vertices if density is None else sample_mesh(src.vertices, src.faces, density)
    pts = pts[torch.isfinite(pts).all(1)]
    n = pts.shape[0]
    if n == 0:
        return dict(max=math.nan, mean=math.nan, rms=math.nan, n=0)
    d = dst.closest(pts, bound).dist
    return dict(max=float(d.max()), mean=float(d.mean()), rms=float(torch.sqrt((d * d).mean())), n=n)


def mesh_deviation(a, b, *, density=None, bound=math.inf):
    """the two-sided deviation between two meshes, each (vertices, faces) or a MeshIndex: for each direction the exact
    distances from the vertices of one mesh -- with `density` from sample_mesh's cloud at that density, vertices included
    -- to the surface of the other.  -> dict(a_to_b=dict(max, mean, rms, n), b_to_a=..., hausdorff=max of the two max).
    `max` is the largest distance over the measured points: a lower bound of the true one-sided Hausdorff distance,
    exact at the samples (the surface between them can lie farther away; a finer density tightens it).  NaN vertices
    are left out; a distance beyond `bound` counts as +inf."""
    bound = _positive(bound, "bound", allow_inf=True)
    if density is not None:
        density = _positive(density, "density")
    ia, ib = _as_index(a, "a"), _as_index(b, "b")
    ab, ba = _one_sided(ia, ib, density, bound), _one_sided(ib, ia, density, bound)
    return dict(a_to_b=ab, b_to_a=ba, hausdorff=max(ab["max"], ba["max"]))


def format_deviation(res, decimals=6):
    """the deviation log, in format_log's style: one line per direction, the symmetric figure, rounded with np.round"""
    def r(v):
        return np.round(np.float64(v), decimals)
    lines = [f"{k} max {r(res[k]['max'])} mean {r(res[k]['mean'])} rms {r(res[k]['rms'])} n {res[k]['n']} \n"
             for k in ("a_to_b", "b_to_a")]
    return "".join(lines) + f"hausdorff {r(res['hausdorff'])} \n"


# ---- the protocols ---------------------------------------------------------------------------------------------------
def _data_cloud(data, density, dev):
    if isinstance(data, (tuple, list)):
        if len(data) != 2:
            raise ValueError("data must be (vertices, faces) or [N, 3] points")
        return sample_mesh(data[0], data[1], density)
    return _points(data, "data", dev, finite=False)


def _metrics(d2s, s2d, max_dist, thresholds):
    def mean_below(d):
        sel = d[d < max_dist]
        return float(sel.mean()) if sel.numel() else math.nan

    mean_d2s, mean_s2d = mean_below(d2s), mean_below(s2d)
    out = dict(mean_d2gt=mean_d2s, mean_gt2d=mean_s2d, over_all=(mean_d2s + mean_s2d) / 2)
    for k, t in enumerate(thresholds, 1):
        p = int((d2s < t).sum()) / d2s.numel()
        r = int((s2d < t).sum()) / s2d.numel()
        out[f"precision_{k}"], out[f"recall_{k}"] = p, r
        out[f"fscore_{k}"] = 2 * p * r / (p + r + 1e-6)
    return out


def vis_colors(dist, vis_dist, max_dist, n=None, where=None):
    """the reference's error colours (float64 RGB in [0, 1]): blue everywhere (n rows), then at rows `where` (all rows
    when None) the red-white ramp R a + W (1 - a), a = min(d, vis_dist) / vis_dist, and green where d >= max_dist"""
    dev = dist.device
    n = dist.numel() if n is None else n
    c = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    c[:, 2] = 1.0
    a = dist.clamp(max=vis_dist) / torch.full_like(dist, vis_dist)   # a true division (torch multiplies by 1 / scalar)
    ramp = torch.stack([1.0 * a + 1.0 * (1 - a), 0.0 * a + 1.0 * (1 - a), 0.0 * a + 1.0 * (1 - a)], -1)
    ramp[dist >= max_dist] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=dev)
    if where is None:
        c[:] = ramp
    else:
        c[where] = ramp
    return c


def _write_vis(vis_dir, name, data_down, data_color, gt, gt_color):
    from .meshing import write_points_ply
    os.makedirs(vis_dir, exist_ok=True)
    write_points_ply(os.path.join(vis_dir, f"vis_{name}_d2gt.ply"), data_down.cpu().numpy(), data_color.cpu().numpy())
    write_points_ply(os.path.join(vis_dir, f"vis_{name}_gt2d.ply"), gt.cpu().numpy(), gt_color.cpu().numpy())


def _check_common(max_dist, thresholds, visualize_threshold):
    max_dist = _positive(max_dist, "max_dist")
    thresholds = tuple(_positive(t, "threshold") for t in thresholds)
    visualize_threshold = _positive(visualize_threshold, "visualize_threshold")
    return max_dist, thresholds, visualize_threshold


def chamfer_deepfashion(data, gt, *, downsample_density=0.002, max_dist=0.1, thresholds=(0.001, 0.002), seed=0,
                        vis_dir=None, name=None, visualize_threshold=0.01):
    """the DeepFashion3D protocol (eval_deepfashion_python.py:62-215).  data: (vertices, faces) (mode mesh) or [N, 3]
    points (mode pcd); gt: [G, 3] points.  -> dict with mean_d2gt, mean_gt2d, over_all, precision_k, recall_k, fscore_k
    (k = 1, 2, ... per threshold), the point counts n_data, n_down, n_gt and thinning_rounds.  vis_dir: also write
    vis_{name}_d2gt.ply / vis_{name}_gt2d.ply there."""
    max_dist, thresholds, vis_t = _check_common(max_dist, thresholds, visualize_threshold)
    density = _positive(downsample_density, "downsample_density")
    if _shape3(gt, "gt").shape[0] == 0:
        raise ValueError("the GT cloud is empty")
    dev = _device(gt, *(data if isinstance(data, (tuple, list)) else (data,)))
    stl = _points(gt, "gt", dev)
    pcd = _data_cloud(data, density, dev)
    if pcd.shape[0] == 0:
        raise ValueError("the data cloud is empty")
    down, info = radius_downsample(pcd, density, seed)
    bound = max(max_dist, *thresholds)
    d2s, _ = nearest(down, stl, bound)
    s2d, _ = nearest(stl, down, bound)
    out = _metrics(d2s, s2d, max_dist, thresholds)
    out.update(n_data=pcd.shape[0], n_down=down.shape[0], n_gt=stl.shape[0], thinning_rounds=info["rounds"])
    if vis_dir is not None:
        _write_vis(vis_dir, name or "000", down, vis_colors(d2s, vis_t, max_dist), stl, vis_colors(s2d, vis_t, max_dist))
    return out


def dtu_masks(data_down, bb, res, obs_mask, patch_size):
    """the reference's DTU selection (eval_dtu_python.py:277-291) in its mixed precision: BB cast to float32, the bounds
    BB[0] - patch and BB[1] + 2 patch computed in float32, compared in float64; grid = around((p - BB[0]) / Res) in
    float64 (half to even) cast to int32.  -> (inbound [K] bool, rows of data_down in data_in_obs [J] int64)"""
    dev = data_down.device
    bb32 = torch.as_tensor(np.asarray(bb, dtype=np.float32).reshape(2, 3), device=dev)
    lo = bb32[0] - torch.tensor(float(patch_size), dtype=torch.float32, device=dev)
    hi = bb32[1] + torch.tensor(float(patch_size) * 2, dtype=torch.float32, device=dev)
    inbound = ((data_down >= lo.double()) & (data_down < hi.double())).all(1)
    rows_in = torch.nonzero(inbound).reshape(-1)
    rel = data_down[rows_in] - bb32[0].double()
    g = torch.round(rel / torch.full_like(rel, float(res))).to(torch.int32)   # not rel * (1 / res): torch's scalar division
    shape = torch.tensor(obs_mask.shape, dtype=torch.int32, device=dev)
    grid_in = ((g >= 0) & (g < shape)).all(1)
    gi = g[grid_in].long()
    in_obs = obs_mask[gi[:, 0], gi[:, 1], gi[:, 2]]
    return inbound, rows_in[grid_in][in_obs]


def above_plane(points, plane):
    """P . (x, y, z, 1) > 0, summed in numpy's order ((P0 x + P1 y) + P2 z) + P3"""
    P = [float(v) for v in np.asarray(plane, dtype=np.float64).reshape(4)]
    s = points[:, 0] * P[0] + points[:, 1] * P[1]
    s = s + points[:, 2] * P[2]
    return (s + P[3] * 1.0) > 0


def chamfer_dtu(data, gt, obs_mask, bb, res, plane, *, downsample_density=0.2, patch_size=60, max_dist=20,
                thresholds=(1, 2), seed=0, vis_dir=None, name=None, visualize_threshold=10):
    """the DTU protocol (eval_dtu_python.py:205-370).  data: (vertices, faces) (mode mesh) or [N, 3] points (mode pcd),
    in world space (mm); gt: [G, 3] STL points; obs_mask [X, Y, Z], bb [2, 3], res, plane [4]: load_dtu_obs.  d2gt runs
    over the down-sampled points inside the ObsMask, gt2d over the GT points above the plane against every down-sampled
    point inside the patch-extended box.  -> dict with mean_d2gt, mean_gt2d, over_all, precision_k, recall_k, fscore_k,
    the point counts n_data, n_down, n_in, n_in_obs, n_gt, n_gt_above and thinning_rounds."""
    max_dist, thresholds, vis_t = _check_common(max_dist, thresholds, visualize_threshold)
    density = _positive(downsample_density, "downsample_density")
    patch_size = float(patch_size)
    if not math.isfinite(patch_size):
        raise ValueError(f"patch_size must be finite (got {patch_size})")
    res = _positive(np.asarray(res, dtype=np.float64).reshape(-1)[0], "res")
    bb = np.asarray(bb)
    if bb.size != 6:
        raise ValueError(f"bb must be [2, 3] (got shape {bb.shape})")
    obs = torch.as_tensor(np.asarray(obs_mask) if not isinstance(obs_mask, torch.Tensor) else obs_mask)
    if obs.dim() != 3:
        raise ValueError(f"obs_mask must be [X, Y, Z] (got {tuple(obs.shape)})")
    if np.asarray(plane).size != 4:
        raise ValueError("plane must hold 4 numbers")
    if _shape3(gt, "gt").shape[0] == 0:
        raise ValueError("the GT cloud is empty")
    dev = _device(gt, *(data if isinstance(data, (tuple, list)) else (data,)))
    obs = obs.to(dev) != 0
    stl = _points(gt, "gt", dev)
    pcd = _data_cloud(data, density, dev)
    if pcd.shape[0] == 0:
        raise ValueError("the data cloud is empty")
    down, info = radius_downsample(pcd, density, seed)
    inbound, rows_obs = dtu_masks(down, bb, res, obs, patch_size)
    data_in = down[inbound]
    data_in_obs = down[rows_obs]
    above = above_plane(stl, plane)
    stl_above = stl[above]
    if data_in_obs.shape[0] == 0:
        raise ValueError("no down-sampled data point lies inside the ObsMask")
    if stl_above.shape[0] == 0:
        raise ValueError("no GT point lies above the ground plane")
    bound = max(max_dist, *thresholds)
    d2s, _ = nearest(data_in_obs, stl, bound)
    s2d, _ = nearest(stl_above, data_in, bound)
    out = _metrics(d2s, s2d, max_dist, thresholds)
    out.update(n_data=pcd.shape[0], n_down=down.shape[0], n_in=data_in.shape[0], n_in_obs=data_in_obs.shape[0],
               n_gt=stl.shape[0], n_gt_above=stl_above.shape[0], thinning_rounds=info["rounds"])
    if vis_dir is not None:
        _write_vis(vis_dir, name or "000", down, vis_colors(d2s, vis_t, max_dist, down.shape[0], rows_obs), stl,
                   vis_colors(s2d, vis_t, max_dist, stl.shape[0], torch.nonzero(above).reshape(-1)))
    return out


def load_dtu_obs(dataset_dir, scan):
    """(obs_mask [X, Y, Z] bool np, bb [2, 3] np, res float, plane [4] float64 np) from
    {dataset_dir}/ObsMask/ObsMask{scan}_10.mat (ObsMask, BB, Res) and Plane{scan}.mat (P), via scipy.io.loadmat"""
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError("load_dtu_obs reads MATLAB files with scipy.io.loadmat: install scipy, or pass obs_mask, bb, "
                          "res and plane to chamfer_dtu directly") from e
    m = loadmat(os.path.join(dataset_dir, "ObsMask", f"ObsMask{scan}_10.mat"))
    p = loadmat(os.path.join(dataset_dir, "ObsMask", f"Plane{scan}.mat"))
    return (np.asarray(m["ObsMask"]).astype(bool), np.asarray(m["BB"]), float(np.asarray(m["Res"]).reshape(-1)[0]),
            np.asarray(p["P"], dtype=np.float64).reshape(4))


# ---- CLI -------------------------------------------------------------------------------------------------------------
def format_log(res, stem, decimals, units="mm"):
    """the reference's log file: three lines of metrics rounded with np.round, then [stem]"""
    def r(k):
        return np.round(np.float64(res[k]), decimals)
    return (f"over_all {r('over_all')} mean_d2gt {r('mean_d2gt')} mean_gt2d {r('mean_gt2d')} \n"
            f"precision_1{units} {r('precision_1')} recall_1{units} {r('recall_1')} fscore_1{units} {r('fscore_1')} \n"
            f"precision_2{units} {r('precision_2')} recall_2{units} {r('recall_2')} fscore_2{units} {r('fscore_2')} \n"
            f"[{stem}] \n")


def parse_log(text):
    """{name: float} of a log written by format_log (the names without the units suffix), plus 'stem'"""
    out = {}
    lines = text.strip().splitlines()
    for ln in lines[:3]:
        tok = ln.split()
        for k, v in zip(tok[::2], tok[1::2]):
            out[k.replace("mm", "")] = float(v)
    out["stem"] = lines[3].strip()[1:-1]
    return out


def _main_deviation(argv):
    from .meshing import read_ply
    ap = argparse.ArgumentParser(prog="python -m neuraludf_amd.evaluation deviation",
                                 description="two-sided exact deviation between two meshes (mesh_deviation)")
    ap.add_argument("--a", type=str, required=True, help="first mesh (PLY with faces)")
    ap.add_argument("--b", type=str, required=True, help="second mesh (PLY with faces)")
    ap.add_argument("--density", type=float, default=None, help="also measure from sample_mesh's points at this density")
    ap.add_argument("--bound", type=float, default=math.inf)
    ap.add_argument("--decimals", type=int, default=6)
    ap.add_argument("--log", type=str, default=None)
    a = ap.parse_args(argv)
    meshes = []
    for path in (a.a, a.b):
        v, f = read_ply(path)
        if f is None:
            raise SystemExit(f"{path} holds no faces")
        meshes.append((torch.as_tensor(np.asarray(v, dtype=np.float64)), torch.as_tensor(np.asarray(f))))
    out = mesh_deviation(meshes[0], meshes[1], density=a.density, bound=a.bound)
    for k in ("a_to_b", "b_to_a"):
        print(f"{k}: max: {out[k]['max']}; mean: {out[k]['mean']}; rms: {out[k]['rms']}; n: {out[k]['n']}.")
    print(f"hausdorff: {out['hausdorff']}")
    log = a.log if a.log is not None else os.path.join(os.path.dirname(a.a), "deviation_result.txt")
    with open(log, "w+") as fh:
        fh.write(format_deviation(out, a.decimals))
    return 0


def _main_intersections(argv):
    from .meshing import read_ply, write_ply
    ap = argparse.ArgumentParser(prog="python -m neuraludf_amd.evaluation intersections",
                                 description="the faces of a mesh that pass through each other, or through another mesh")
    ap.add_argument("--mesh", type=str, required=True, help="the mesh (PLY with faces)")
    ap.add_argument("--other", type=str, default=None, help="a second mesh: its faces against the first's")
    ap.add_argument("--out", type=str, default=None, help="write the mesh with its flagged faces coloured (PLY)")
    a = ap.parse_args(argv)
    meshes = []
    for path in (a.mesh, a.other):
        if path is None:
            continue
        v, f = read_ply(path)
        if f is None:
            raise SystemExit(f"{path} holds no faces")
        meshes.append((torch.as_tensor(np.asarray(v, dtype=np.float64)), torch.as_tensor(np.asarray(f))))
    if a.other is None:
        res = self_intersections(*meshes[0])
        mask = res.face_mask
    else:
        res = mesh_intersections(meshes[0], meshes[1])
        mask = res.mask_a
    counts = {name: int((res.kind == k).sum()) for name, k in ISECT_KINDS.items()}
    print(f"pairs: {res.pairs.shape[0]}; " + "; ".join(f"{k}: {v}" for k, v in counts.items())
          + f"; flagged faces: {int(mask.sum())} of {mask.numel()}.")
    if a.out is not None:
        # a vertex of a flagged face is red, the others grey (PLY colours live on vertices)
        v, f = meshes[0]
        flagged = torch.zeros(v.shape[0], dtype=torch.bool)
        flagged[f.to(torch.int64)[mask.cpu()].reshape(-1)] = True
        colors = np.where(flagged.numpy()[:, None], np.array([[255, 0, 0]], np.uint8), np.array([[160, 160, 160]], np.uint8))
        write_ply(a.out, v.numpy(), f.numpy(), colors=colors)
    return 0


def _main_winding(argv):
    from .meshing import read_ply
    ap = argparse.ArgumentParser(prog="python -m neuraludf_amd.evaluation winding",
                                 description="generalised winding numbers of a mesh at points or on a grid (winding_number)")
    ap.add_argument("--mesh", type=str, required=True, help="the mesh (PLY with faces)")
    where = ap.add_mutually_exclusive_group(required=True)
    where.add_argument("--points", type=str, default=None, help="the query points (PLY)")
    where.add_argument("--grid", type=int, default=None, help="N: N^3 points spanning the mesh's box, x outermost")
    ap.add_argument("--out", type=str, required=True, help="the winding numbers (.npy: [M], or [N, N, N] with --grid)")
    ap.add_argument("--beta", type=float, default=WINDING_BETA)
    ap.add_argument("--orient", action="store_true", help="run meshclean.orient_faces on the mesh first")
    a = ap.parse_args(argv)
    v, f = read_ply(a.mesh)
    if f is None:
        raise SystemExit(f"{a.mesh} holds no faces")
    v, f = torch.as_tensor(np.asarray(v, dtype=np.float64)), torch.as_tensor(np.asarray(f))
    if a.orient:
        from .meshclean import orient_faces          # meshclean imports this module
        f = orient_faces(v.cuda(), f.to(torch.int64).cuda()).faces
    index = MeshIndex(v, f)
    if a.grid is not None:
        if a.grid < 1:
            raise SystemExit("--grid needs N >= 1")
        axes = [torch.linspace(l, h, a.grid, dtype=torch.float64) for l, h in zip(index.lo, index.hi)]
        pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    else:
        pts = torch.as_tensor(np.asarray(read_ply(a.points)[0], dtype=np.float64))
    w = index.winding(pts, a.beta).cpu().numpy()
    if a.grid is not None:
        w = w.reshape(a.grid, a.grid, a.grid)
    np.save(a.out, w)
    inside = int((np.abs(w) > 0.5).sum())
    print(f"points: {w.size}; inside (|w| > 0.5): {inside}; min: {w.min() if w.size else math.nan}; "
          f"max: {w.max() if w.size else math.nan}.")
    return 0


def main(argv=None):
    from pathlib import Path
    from .meshing import read_ply
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "winding":
        return _main_winding(argv[1:])
    if argv and argv[0] == "deviation":            # the third protocol word has arguments of its own
        return _main_deviation(argv[1:])
    if argv and argv[0] == "intersections":
        return _main_intersections(argv[1:])
    ap = argparse.ArgumentParser(prog="python -m neuraludf_amd.evaluation", description=__doc__.split("\n\n")[0])
    ap.add_argument("protocol", choices=sorted(PROTOCOLS))
    ap.add_argument("--data", type=str, default="data_in.ply")
    ap.add_argument("--gt", type=str, required=True, help="ground truth")
    ap.add_argument("--scan", type=int, default=1)
    ap.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    ap.add_argument("--dataset_dir", type=str, default=None, help="DTU: the directory holding ObsMask/")
    ap.add_argument("--vis_out_dir", type=str, default=".")
    ap.add_argument("--no_vis", action="store_true", help="do not write the visualisation clouds")
    ap.add_argument("--downsample_density", type=float, default=None)
    ap.add_argument("--patch_size", type=float, default=None)
    ap.add_argument("--max_dist", type=float, default=None)
    ap.add_argument("--visualize_threshold", type=float, default=None)
    ap.add_argument("--log", type=str, default=None)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    proto = PROTOCOLS[a.protocol]
    for k in ("downsample_density", "patch_size", "max_dist", "visualize_threshold"):
        if getattr(a, k) is None:
            setattr(a, k, proto[k])
    v, f = read_ply(a.data)
    if a.mode == "mesh":
        if f is None:
            raise SystemExit(f"{a.data} holds no faces: use --mode pcd")
        data = (v, f)
    else:
        data = v
    gt, _ = read_ply(a.gt)
    kw = dict(downsample_density=a.downsample_density, max_dist=a.max_dist, thresholds=proto["thresholds"], seed=a.seed,
              vis_dir=None if a.no_vis else a.vis_out_dir, name=f"{a.scan:03}", visualize_threshold=a.visualize_threshold)
    if a.protocol == "dtu":
        if a.dataset_dir is None:
            raise SystemExit("dtu needs --dataset_dir (the directory holding ObsMask/)")
        obs, bb, res, plane = load_dtu_obs(a.dataset_dir, a.scan)
        out = chamfer_dtu(data, gt, obs, bb, res, plane, patch_size=a.patch_size, **kw)
    else:
        out = chamfer_deepfashion(data, gt, **kw)
    print(f"over_all: {out['over_all']}; mean_d2gt: {out['mean_d2gt']}; mean_gt2d: {out['mean_gt2d']}.")
    print(f"precision_1mm: {out['precision_1']};  recall_1mm: {out['recall_1']};  fscore_1mm: {out['fscore_1']}")
    print(f"precision_2mm: {out['precision_2']};  recall_2mm: {out['recall_2']};  fscore_2mm: {out['fscore_2']}")
    path = Path(a.data)
    log = a.log if a.log is not None else os.path.join(str(path.parent), "eval_result.txt")
    with open(log, "w+") as fh:
        fh.write(format_log(out, path.stem, proto["decimals"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
