"""Open-surface meshes of the UDF on the GPU (MeshUDF, Guillard et al. 2022): what the reference's
Runner.extract_udf_mesh (exp_runner_blending.py:763-800) gets from extract_mesh.get_mesh_udf_fast (extract_mesh.py:169-354)
and its serial Cython mesher.

    grid      udf_grid            UDF values on the dense grid, UDF gradients where U < grad_band * h
    mesh      udf_marching_cubes  three HIP launches (csrc/meshudf.hip) and deterministic torch integer scans between them
                                  (_mesh_dense, the driver of every dense mesher; _mesh_sparse is that of the sparse ones:
                                  one kernel set, csrc/mc_pipeline.h, under a MeshUDF and a level-set rule)
    sparse    udf_sparse_grid, udf_marching_cubes_sparse   the same mesh from the B^3-cell blocks near the surface only
                                  (csrc/meshudf_sparse.hip): queries and memory grow with the surface, N up to 4096;
                                  _select_and_query builds the bricks of both sparse grids (_SparseGrid)
    level set iso_marching_cubes, iso_sparse_grid, iso_marching_cubes_sparse, extract_iso_mesh   the surface {F = level}
                                  of a signed or unsigned field (csrc/isosurface.hip): what the reference's
                                  extract_geometry gets from PyMCubes, and the zero set of SDF networks
    filter    filter_mesh         the reference's post-steps (extract_mesh.py:205-222) without trimesh
    clean-up  neuraludf_amd.meshclean (re-exported here): fill_holes, smooth_borders, filter_components, clean_dtu_mesh ...
    simplify  simplify_mesh, simplify_to_faces (meshclean, csrc/meshsimplify.hip): vertex clustering on a uniform grid,
                                  each cluster's vertex placed by quadric error minimisation with boundary quadrics
    measure   simplify_to_error, transfer_attributes (meshclean), evaluation.closest_on_mesh / mesh_deviation
                                  (csrc/meshdist.hip): exact point-to-mesh distance, simplification to a measured error,
                                  attributes carried to the closest point of another mesh
    smooth    smooth_mesh, denoise_mesh (meshclean, csrc/meshsmooth.hip): Taubin smoothing and bilateral normal denoising
                                  of the grid noise the mesher leaves, before the simplification freezes it
    subdivide subdivide_mesh, subdivide_to_edge (meshclean, csrc/meshsubdiv.hip): Loop and midpoint subdivision, and
                                  midpoint splits of the edges above a length, after the simplification: vertex density
                                  is the resolution of vertex colours
    remesh    remesh_isotropic (meshclean, csrc/meshremesh.hip): split, collapse, flip, relax and project towards
                                  well-shaped triangles of a requested edge length
    crossings close_holes_checked, drop_self_intersections (meshclean; evaluation.self_intersections,
              csrc/meshintersect.hip): patches that cut through the surface taken back, crossing and folded faces dropped
    holes     border_loops, close_holes (meshclean, csrc/meshhole.hip): the border as canonical loops and chains, and the
                                  loops of up to 64 edges closed with their minimum-area triangulation (fill_holes stops
                                  at 4 edges)
    winding   orient_faces, vertex_normals (meshclean, csrc/meshorient.hip): consistent winding per component and
                                  angle-weighted normals; the mesher's own winding is decided cell by cell
    file      write_ply           binary little-endian PLY, with normals and colours when given
              write_obj, read_obj OBJ / MTL / PNG of a textured mesh
    drawing   neuraludf_amd.meshrender: depth / face / normal maps from the dataset cameras, depth-tested visibility and
                                  vertex colours from the source images (csrc/meshraster.hip); texture atlases baked
                                  from them (csrc/meshtexture.hip)

    python -m neuraludf_amd.meshing IN.ply OUT.ply [--fill-holes] [--smooth-borders] [--min-faces N | --keep-largest]
                                    [--border-loops] [--close-holes N [--close-holes-perimeter P]]
                                    [--dtu-dir D --scan N [--mask-dilated-size 11] [--minimal-vis 2]]
                                    [--denoise [--sigma-s S]] [--smooth N [--smooth-weights uniform|cotangent]]
                                    [--free-boundary]
                                    [--simplify CELL | --simplify-to FACES | --simplify-max-error E]
                                    [--remesh L [--remesh-iterations N]]
                                    [--max-edge H] [--subdivide N [--subdivide-scheme loop|midpoint]]
                                    [--orient | --outward-from X Y Z] [--normals] [--colour] [--render DIR]
                                    [--texture OUT.obj [--texture-size N | --texture-density D]]

The signs of a cell's corners are chosen inside the cell alone (no propagation between cells): the corner of largest U
is `+`, every other corner is `+` iff its gradient has a non-negative float64 dot product with that corner's.  A cell is
active when the mean of its corner values is < 1.05 h and their max <= 1.74 h (h: the largest grid spacing), the
reference's thresholds.  The case table is generated by neuraludf_amd/mc_tables.py.  Vertices are ordered by edge id
(3 lin(lower end) + axis), faces by cell and table order: the mesh is identical from run to run.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, meshclean, meshrender
from ._lib import call, ptr
from .meshclean import (EdgeTable, Orientation, Simplified, boundary_degree, clean_by_views, clean_dtu_mesh,  # noqa: F401
                        compact_mesh, denoise_mesh, dilate_masks, ellipse_footprint, face_components, fill_holes,
                        filter_components, load_dtu_views, mesh_edges, orient_faces, simplify_mesh, simplify_to_error,
                        simplify_to_faces, smooth_borders, smooth_mesh, transfer_attributes, vertex_adjacency,
                        vertex_normals, view_counts)
from .meshclean import Subdivided, subdivide_mesh, subdivide_to_edge  # noqa: F401
from .meshclean import Remeshed, remesh_isotropic  # noqa: F401
from .meshclean import BorderLoops, ClosedHoles, border_loops, close_holes  # noqa: F401
from .meshclean import close_holes_checked, drop_self_intersections  # noqa: F401
from .models import udf_renderer_blending as rb

MIN_N, MAX_N = 3, 1024
MEAN_RATIO, MAX_RATIO = 1.05, 1.74          # active-cell thresholds in units of h (_marching_cubes_lewiner_cy.pyx:1157-1158)
SCAN_CHUNK = 1 << 30                         # elements per torch scan / compaction call over the per-edge flags
SPARSE_MIN_N, SPARSE_MAX_N = 3, 4096         # sparse extraction: edge ids 3 N^3 and cell ids fit int64, block ids int32
SPARSE_BLOCKS = (4, 8)                       # cells per block and axis


def grid_spacing(bound_min, bound_max, resolution) -> float:
    """h: the largest grid spacing of the box, in float64"""
    n = int(resolution)
    return max((float(bound_max[a]) - float(bound_min[a])) / (n - 1) for a in range(3))


def thresholds(h):
    """(mean, max) thresholds of the active-cell test, as the fp32 values the kernel compares with"""
    return np.float32(MEAN_RATIO * h), np.float32(MAX_RATIO * h)


def _check_n(n):
    if not MIN_N <= n <= MAX_N:
        raise ValueError(f"grid resolution {n} outside [{MIN_N}, {MAX_N}]")


def _device_of(module):
    return next(module.parameters()).device


@torch.no_grad()
def udf_grid(udf_network, resolution, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), grad_band=2.0):
    """-> (U [N, N, N] fp32, G [N, N, N, 3] fp32), device tensors on the network's device.  U is the UDF on the grid of
    extract_fields (same slab-wise query), clamped at 0 as the reference does (extract_mesh.py:198); G is
    `udf_network.gradient` at the points with U < grad_band * h only (compacted, in chunks, extract_mesh.py:76-95) and 0
    elsewhere -- every corner of an active cell (max <= 1.74 h) lies in that band."""
    n = int(resolution)
    _check_n(n)
    U = udf_values(udf_network, n, bound_min, bound_max)
    return U, udf_gradients_in_band(udf_network, U, bound_min, bound_max, grad_band)


@torch.no_grad()
def udf_values(udf_network, resolution, bound_min, bound_max):
    """U of `udf_grid`"""
    dev = _device_of(udf_network)
    return rb._grid_query_device(bound_min, bound_max, int(resolution), lambda p: udf_network.udf(p)[:, 0], dev,
                                 1).clamp_min_(0.0)


@torch.no_grad()
def udf_gradients_in_band(udf_network, U, bound_min, bound_max, grad_band=2.0):
    """G of `udf_grid` for its U"""
    n = U.shape[0]
    h = grid_spacing(bound_min, bound_max, n)
    G = torch.zeros((n, n, n, 3), dtype=torch.float32, device=U.device)
    idx = torch.nonzero(U.reshape(-1) < grad_band * h).reshape(-1)
    _query_gradients(udf_network, rb._grid_axes(bound_min, bound_max, n, U.device), idx, n, G.view(-1, 3), idx)
    return G


def _node_points(axes, lin, n):
    """coordinates of the grid nodes with linear ids `lin`, taken from the axes by index as the dense path does"""
    return torch.stack([axes[0][lin // (n * n)], axes[1][(lin // n) % n], axes[2][lin % n]], -1)


def _query_nodes(query_func, axes, lin, n, dev):
    """fp32 values of query_func(pts [P, 3]) -> [P] at the grid nodes with linear ids `lin` (a tensor, or a count: every id
    below it), in chunks"""
    count = lin if isinstance(lin, int) else lin.numel()
    out = torch.empty(count, dtype=torch.float32, device=dev)
    for s in range(0, count, rb.GRID_CHUNK_POINTS):
        e = min(s + rb.GRID_CHUNK_POINTS, count)
        i = torch.arange(s, e, device=dev) if isinstance(lin, int) else lin[s:e]
        out[s:e] = query_func(_node_points(axes, i, n)).detach().reshape(-1)
    return out


def _query_gradients(udf_network, axes, lin, n, out, rows):
    """out[rows] = udf_network.gradient at the grid nodes with linear ids `lin` (one per row), in chunks"""
    chunk = rb.GRID_CHUNK_POINTS // 4                          # gradient queries keep activations (as _grid_query)
    for s in range(0, rows.numel(), chunk):
        out[rows[s:s + chunk]] = udf_network.gradient(_node_points(axes, lin[s:s + chunk], n)).reshape(-1, 3).detach()


def _empty_mesh(dev):
    return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev)


def _nonzero(flags):
    """ascending indices of the non-zero entries of a 1-D tensor (int64), in chunks of at most SCAN_CHUNK elements"""
    parts = [torch.nonzero(flags[s:s + SCAN_CHUNK]).reshape(-1) + s for s in range(0, flags.numel(), SCAN_CHUNK)]
    return torch.cat(parts) if parts else flags.new_zeros(0, dtype=torch.int64)


def _inclusive_scan(flags):
    """int64 inclusive prefix sum of a 1-D uint8 tensor, in chunks of at most SCAN_CHUNK elements"""
    out = torch.empty(flags.numel(), dtype=torch.int64, device=flags.device)
    carry = None
    for s in range(0, flags.numel(), SCAN_CHUNK):
        part = out[s:s + SCAN_CHUNK]
        torch.cumsum(flags[s:s + SCAN_CHUNK], 0, dtype=torch.int64, out=part)
        if carry is not None:
            part += carry
        carry = part[-1]
    return out


def _stage_marker(events):
    """mark(name) ends the open stage and starts `name` (None: ends the last one); a no-op without an event dict"""
    if events is None:
        return lambda name: None
    state = {}

    def mark(name):
        if "open" in state:
            events[state["open"]][1].record()
        if name is not None:
            events[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            events[name][0].record()
            state["open"] = name
    return mark


def _face_offsets(ntri, cells):
    """-> (exclusive prefix sum of the triangle counts ntri[cells] (int64), their total)"""
    counts = ntri[cells].to(torch.int64)
    ends = torch.cumsum(counts, 0)
    return ends - counts, int(ends[-1]) if cells.numel() else 0


def _mesh_dense(d, prefix, n, dev, events):
    """the dense pipeline (csrc/mc_pipeline.h) of the mesher whose entry points start with `prefix`, on a grid of n nodes
    per axis: classify, the torch integer scans, emit, vertices.  `d`: the descriptor with the field, the axes, N and the
    rule's parameters set; the buffers every mesher has are added here.  -> (verts [V, 3] fp32, faces [F, 3] int64)"""
    case = torch.empty((n - 1) ** 3, dtype=torch.uint8, device=dev)
    ntri = torch.empty((n - 1) ** 3, dtype=torch.uint8, device=dev)
    flags = torch.zeros(3 * n ** 3, dtype=torch.uint8, device=dev)
    d.cell_case, d.cell_ntri, d.edge_flag = ptr(case), ptr(ntri), ptr(flags)
    mark = _stage_marker(events)
    mark("classify")
    call(prefix + "classify", d)
    mark("scan")
    cells = _nonzero(ntri)
    face_off, n_faces = _face_offsets(ntri, cells)
    edges = _nonzero(flags)
    edge_scan = _inclusive_scan(flags)
    del flags
    faces = torch.empty((n_faces, 3), dtype=torch.int64, device=dev)
    verts = torch.empty((edges.numel(), 3), dtype=torch.float32, device=dev)
    d.cells, d.face_off, d.edge_scan, d.faces = ptr(cells), ptr(face_off), ptr(edge_scan), ptr(faces)
    d.edges, d.verts = ptr(edges), ptr(verts)
    d.n_cells, d.n_edges, d.n_faces = cells.numel(), edges.numel(), n_faces
    mark("emit")
    call(prefix + "emit", d)
    mark("vertices")
    call(prefix + "vertices", d)
    mark(None)
    return verts, faces


def udf_marching_cubes(U, G, bound_min, bound_max, _events=None):
    """MeshUDF marching cubes of a UDF grid (csrc/meshudf.hip) -> (verts [V, 3] fp32, faces [F, 3] int64), device
    tensors, unfiltered.  U: [N, N, N] fp32 >= 0 and G: [N, N, N, 3] fp32 on one GPU, on the grid
    linspace(bound_min, bound_max, N) per axis (x-major).  Only the direction of G matters.  Empty inputs and fields with
    no surface give empty outputs.  (`_events`: a dict that receives a pair of recorded torch.cuda.Events around each
    stage -- classify, scan, emit, vertices -- for scripts/bench_meshudf.py.)"""
    if not isinstance(U, torch.Tensor) or not isinstance(G, torch.Tensor):
        raise ValueError("U and G must be torch tensors")
    if U.dtype != torch.float32 or G.dtype != torch.float32:
        raise ValueError(f"U and G must be float32 (got {U.dtype}, {G.dtype})")
    if not U.is_cuda or G.device != U.device:
        raise ValueError(f"U and G must be on the same GPU (got {U.device}, {G.device})")
    if U.dim() != 3 or not U.shape[0] == U.shape[1] == U.shape[2]:
        raise ValueError(f"U must be [N, N, N] (got {tuple(U.shape)})")
    n, dev = U.shape[0], U.device
    if tuple(G.shape) != (n, n, n, 3):
        raise ValueError(f"G must be [{n}, {n}, {n}, 3] like U (got {tuple(G.shape)})")
    if n == 0:
        return _empty_mesh(dev)
    _check_n(n)
    U, G = U.contiguous(), G.contiguous()
    axes = rb._grid_axes(bound_min, bound_max, n, dev).contiguous()
    mean_thr, max_thr = thresholds(grid_spacing(bound_min, bound_max, n))
    d = _lib.MeshUDF(U=ptr(U), G=ptr(G), axes=ptr(axes), N=n, mean_thr=float(mean_thr), max_thr=float(max_thr))
    return _mesh_dense(d, "nudf_meshudf_", n, dev, _events)


# ---- sparse extraction: only the blocks near the surface are queried at full resolution, stored and meshed -------------

def _check_sparse(n, block, lipschitz):
    if block not in SPARSE_BLOCKS:
        raise ValueError(f"block {block!r} is not one of {SPARSE_BLOCKS}")
    if isinstance(lipschitz, (bool, str)) or not isinstance(lipschitz, (int, float, np.floating)) \
            or not math.isfinite(lipschitz) or lipschitz <= 0:
        raise ValueError(f"lipschitz {lipschitz!r} is not a finite positive number")
    if not SPARSE_MIN_N <= n <= SPARSE_MAX_N:
        raise ValueError(f"grid resolution {n} outside [{SPARSE_MIN_N}, {SPARSE_MAX_N}]")


def sparse_threshold(bound_min, bound_max, resolution, block, lipschitz):
    """the block-selection threshold 1.74 h + lipschitz r (r: half the diagonal of a block of `block` cells per axis),
    evaluated in float64 and rounded up to the fp32 value the coarse minima are compared with"""
    n = int(resolution)
    ha = [(float(bound_max[a]) - float(bound_min[a])) / (n - 1) for a in range(3)]
    t = MAX_RATIO * max(ha) + float(lipschitz) * (0.5 * math.sqrt(sum((block * x) ** 2 for x in ha)))
    f = np.float32(t)
    return f if float(f) >= t else np.nextafter(f, np.float32(np.inf))


def _brick_node_ids(blocks, n, block, nb):
    """[K, (B+1)^3] int64 linear node ids of the bricks of `blocks`, -1 at the padding past the grid's end"""
    p1 = block + 1
    loc = torch.arange(p1 ** 3, device=blocks.device)
    ids, valid = 0, True
    for b, a in ((blocks // (nb * nb), loc // (p1 * p1)), ((blocks // nb) % nb, (loc // p1) % p1), (blocks % nb, loc % p1)):
        x = (b * block)[:, None] + a[None, :]
        valid = (x < n) & valid
        ids = ids * n + x
    return torch.where(valid, ids, -1)


class _SparseGrid:
    """the selected blocks of a grid and the bricks stored on them: N, B, nb, bound_min, bound_max, axes [3, N]; blocks [K]
    ascending linear block ids (int64), block_slot [nb^3] int32 (-1: not selected); per name in BRICKS an fp32 brick array
    [K, (B+1)^3, ...] (local index (ax (B+1) + ay) (B+1) + az; nodes past the grid's end are padding, never read as cell
    corners); coarse [(nb+1)^3] the coarse-node values the selection saw; the counters n_coarse, n_blocks and n_queried
    (unique fine nodes)."""
    BRICKS = {}                                  # name -> (trailing shape, value at the padding and outside every brick)

    def __init__(self, N, B, nb, bound_min, bound_max, axes, blocks, block_slot, coarse, n_queried):
        self.N, self.B, self.nb = int(N), int(B), int(nb)
        self.bound_min, self.bound_max = tuple(float(x) for x in bound_min), tuple(float(x) for x in bound_max)
        self.axes, self.blocks, self.block_slot, self.coarse = axes, blocks, block_slot, coarse
        self.n_coarse, self.n_blocks, self.n_queried = (self.nb + 1) ** 3, int(blocks.numel()), int(n_queried)

    def node_ids(self):
        """[K, (B+1)^3] int64 linear grid-node id (i N + j) N + k of every brick node, -1 at the padding"""
        return _brick_node_ids(self.blocks, self.N, self.B, self.nb)

    def _dense(self):
        """one dense [N, N, N, ...] volume per brick array, holding the brick values and the padding value at every node
        that is in no brick; N <= 1024 only (the dense mesher's limit)"""
        n = self.N
        if n > MAX_N:
            raise ValueError(f"to_dense: grid resolution {n} above {MAX_N}")
        bricks = [getattr(self, name) for name in self.BRICKS]
        out = [torch.full((n, n, n) + tail, fill, dtype=torch.float32, device=bricks[0].device)
               for tail, fill in self.BRICKS.values()]
        if self.n_blocks:
            ids = self.node_ids().reshape(-1)
            keep = ids >= 0
            ids = ids[keep]
            for vol, brick, (tail, _) in zip(out, bricks, self.BRICKS.values()):
                vol.view(-1, *tail)[ids] = brick.reshape(-1, *tail)[keep]          # copies of a shared node hold the same bits
        return out


class SparseUDFGrid(_SparseGrid):
    """the UDF on the selected blocks of a grid (`udf_sparse_grid`): N, B, nb, bound_min, bound_max, axes [3, N];
    blocks [K] ascending linear block ids (int64), block_slot [nb^3] int32 (-1: not selected); bricks U [K, (B+1)^3] and
    G [K, (B+1)^3, 3] fp32 (local index (ax (B+1) + ay) (B+1) + az; nodes past the grid's end are padding: U = +inf,
    G = 0, never read as cell corners); coarse [(nb+1)^3] the coarse-node values the selection saw; the counters n_coarse,
    n_blocks, n_queried (unique fine nodes) and n_grad (nodes whose gradient was queried)."""
    BRICKS = {"U": ((), float("inf")), "G": ((3,), 0.0)}

    def __init__(self, N, B, nb, bound_min, bound_max, axes, blocks, block_slot, U, G, coarse=None, n_queried=0, n_grad=0):
        super().__init__(N, B, nb, bound_min, bound_max, axes, blocks, block_slot, coarse, n_queried)
        self.U, self.G, self.n_grad = U, G, int(n_grad)

    def to_dense(self):
        """-> (U [N, N, N], G [N, N, N, 3]) dense volumes holding the brick values, U = +inf and G = 0 at every node
        that is in no brick; N <= 1024 only (the dense mesher's limit)"""
        return tuple(self._dense())


class SparseFieldGrid(_SparseGrid):
    """a scalar field on the selected blocks of a grid (`iso_sparse_grid`), the storage of SparseUDFGrid without
    gradients: N, B, nb, bound_min, bound_max, axes [3, N]; blocks [K] ascending linear block ids (int64), block_slot
    [nb^3] int32 (-1: not selected); bricks F [K, (B+1)^3] fp32 (local index (ax (B+1) + ay) (B+1) + az; nodes past the
    grid's end are padding: +inf, never read as cell corners); coarse [(nb+1)^3] the coarse-node values the selection saw;
    the counters n_coarse, n_blocks and n_queried (unique fine nodes)."""
    BRICKS = {"F": ((), float("inf"))}

    def __init__(self, N, B, nb, bound_min, bound_max, axes, blocks, block_slot, F, coarse=None, n_queried=0):
        super().__init__(N, B, nb, bound_min, bound_max, axes, blocks, block_slot, coarse, n_queried)
        self.F = F

    def to_dense(self):
        """-> F [N, N, N]: the brick values, +inf (no cell that touches it emits) at every node that is in no brick;
        N <= 1024 only (the dense mesher's limit)"""
        return self._dense()[0]


def _block_corners(c, op):
    """op (torch.minimum or torch.maximum, both propagate NaN) over the eight coarse corners [nb+1]^3 of every block"""
    nb = c.shape[0] - 1
    out = c[:-1, :-1, :-1]
    for dx, dy, dz in [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]:
        out = op(out, c[dx:dx + nb, dy:dy + nb, dz:dz + nb])
    return out


def _select_and_query(query_func, select, clamp_min, n, block, bound_min, bound_max, dev, mark):
    """the stages coarse, select and fine of a sparse grid: query_func(pts [P, 3]) -> [P] at the (nb+1)^3 coarse nodes
    min(b block, N-1), the blocks where select(coarse values [nb+1, nb+1, nb+1]) -> bool [nb, nb, nb] holds, and the
    field at the sorted unique nodes of their bricks (each is queried once).  Coarse and fine values are clamped from
    below at `clamp_min` unless it is None.  -> (geometry: the constructor arguments N ... block_slot of a grid by name,
    coarse, nodes, vals, scatter); scatter(per-node values, fill) -> brick array [K, (B+1)^3, ...], `fill` at the padding"""
    nb = -(-(n - 1) // block)
    axes = rb._grid_axes(bound_min, bound_max, n, dev).contiguous()
    mark("coarse")
    c1 = nb + 1
    caxes = axes[:, (torch.arange(c1, device=dev) * block).clamp_max_(n - 1)]
    coarse = _query_nodes(query_func, caxes, c1 ** 3, c1, dev)
    if clamp_min is not None:
        coarse.clamp_min_(clamp_min)
    mark("select")
    blocks = torch.nonzero(select(coarse.view(c1, c1, c1)).reshape(-1)).reshape(-1)
    k = blocks.numel()
    block_slot = torch.full((nb ** 3,), -1, dtype=torch.int32, device=dev)
    block_slot[blocks] = torch.arange(k, dtype=torch.int32, device=dev)
    ids = _brick_node_ids(blocks, n, block, nb).reshape(-1)
    keep = ids >= 0
    nodes, inv = torch.unique(ids[keep], return_inverse=True)            # ascending node ids: each is queried once
    del ids
    mark("fine")
    vals = _query_nodes(query_func, axes, nodes, n, dev)
    if clamp_min is not None:
        vals.clamp_min_(clamp_min)

    def scatter(per_node, fill):
        out = torch.full((keep.numel(),) + per_node.shape[1:], fill, dtype=torch.float32, device=dev)
        out[keep] = per_node[inv]
        return out.view(k, (block + 1) ** 3, *per_node.shape[1:])
    geometry = dict(N=n, B=block, nb=nb, bound_min=bound_min, bound_max=bound_max, axes=axes, blocks=blocks,
                    block_slot=block_slot)
    return geometry, coarse, nodes, vals, scatter


@torch.no_grad()
def udf_sparse_grid(udf_network, resolution, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), block=8,
                    lipschitz=2.0, grad_band=2.0, device=None, _events=None):
    """-> SparseUDFGrid: the values `udf_grid` would hold, on the blocks of `block`^3 cells that can contain an active
    cell only.  `udf_network`: any object with .udf(pts) -> [P, 1] and .gradient(pts) reshapeable to [P, 3]; `device`
    defaults to the device of its parameters.  The grid and its point coordinates are the dense path's.

    Selection: nb = ceil((N-1) / block) blocks per axis; the UDF is queried at the (nb+1)^3 coarse nodes min(b block, N-1);
    a block is selected iff the minimum of its eight coarse corners (clamped at 0; a NaN corner counts as +inf) is
    <= 1.74 h + lipschitz r, r = half the block's diagonal (`sparse_threshold`).  Every point of a block lies within r of
    a corner and every corner of an active cell is <= 1.74 h, so with |grad U| <= lipschitz no active cell is lost.
    `lipschitz` is a safety parameter, not a measurement: a field steeper than it can lose cells (the geometric init
    reaches 1.22 in the band, eikonal-trained networks sit near 1; the default 2.0 leaves room).

    Every grid node of a selected block is queried exactly once (sorted unique node ids), so all brick copies of a shared
    node hold the same bits and block faces cannot crack; gradients are queried where U < grad_band h and are 0
    elsewhere, as in the dense path.  No allocation is O(N^3); the coarse values and block_slot are O((N / block)^3).
    (`_events`: stage events for scripts/bench_meshudf_sparse.py, as in `udf_marching_cubes`.)"""
    n = int(resolution)
    _check_sparse(n, block, lipschitz)
    dev = torch.device(device) if device is not None else _device_of(udf_network)
    thr = torch.tensor(sparse_threshold(bound_min, bound_max, n, block, lipschitz), device=dev)
    mark = _stage_marker(_events)

    def select(c):
        return _block_corners(torch.nan_to_num(c, nan=float("inf"), posinf=float("inf")), torch.minimum) <= thr
    geometry, coarse, nodes, vals, scatter = _select_and_query(lambda p: udf_network.udf(p)[:, 0], select, 0.0, n, block,
                                                               bound_min, bound_max, dev, mark)
    mark("gradient")
    band = torch.nonzero(vals < grad_band * grid_spacing(bound_min, bound_max, n)).reshape(-1)
    grads = torch.zeros((nodes.numel(), 3), dtype=torch.float32, device=dev)
    _query_gradients(udf_network, geometry["axes"], nodes[band], n, grads, band)
    mark("bricks")
    U, G = scatter(vals, float("inf")), scatter(grads, 0.0)
    mark(None)
    return SparseUDFGrid(**geometry, U=U, G=G, coarse=coarse, n_queried=nodes.numel(), n_grad=band.numel())


def _mesh_sparse(grid, desc, prefix, events, check_nb):
    """the sparse pipeline (csrc/mc_pipeline.h) of the mesher whose entry points start with `prefix` over the bricks of
    `grid`: classify, the torch integer sorts over the cells with triangles and their edge ids, emit, vertices.
    desc(**fields) -> the descriptor: the caller adds the rule's parameters to the fields every mesher has.  check_nb: also
    refuse a grid whose nb is not ceil((N-1) / B) here (the library refuses it in any case).
    -> (verts [V, 3] fp32, faces [F, 3] int64)"""
    n, b, nb, k = grid.N, grid.B, grid.nb, grid.n_blocks
    _check_sparse(n, b, 1.0)
    bricks = {name: getattr(grid, name) for name in grid.BRICKS}
    dev = next(iter(bricks.values())).device
    if k == 0:
        return _empty_mesh(dev)
    p, c, m = (b + 1) ** 3, b ** 3, n - 1
    if any(tuple(t.shape) != (k, p) + grid.BRICKS[name][0] for name, t in bricks.items()) \
            or grid.block_slot.numel() != nb ** 3 or (check_nb and nb != -(-m // b)):
        raise ValueError("grid: brick storage does not match its blocks")
    if any(t.dtype != torch.float32 for t in bricks.values()) or grid.block_slot.dtype != torch.int32 \
            or grid.blocks.dtype != torch.int64:
        raise ValueError(f"grid: {' and '.join(bricks)} must be float32, block_slot int32, blocks int64")
    bricks = {name: t.contiguous() for name, t in bricks.items()}
    axes, blocks, block_slot = grid.axes.contiguous(), grid.blocks.contiguous(), grid.block_slot.contiguous()
    case = torch.empty(k * c, dtype=torch.uint8, device=dev)
    ntri = torch.empty(k * c, dtype=torch.uint8, device=dev)
    d = desc(axes=ptr(axes), blocks=ptr(blocks), block_slot=ptr(block_slot), cell_case=ptr(case), cell_ntri=ptr(ntri),
             n_blocks=k, N=n, B=b, nb=nb, **{name: ptr(t) for name, t in bricks.items()})
    mark = _stage_marker(events)
    mark("classify")
    call(prefix + "classify", d)
    mark("sort")
    t = _nonzero(ntri)                                        # brick cells with triangles -> their global cell indices
    blk, lc = blocks[t // c], t % c
    cell = (((blk // (nb * nb)) * b + lc // (b * b)) * m + ((blk // nb) % nb) * b + (lc // b) % b) * m \
        + (blk % nb) * b + lc % b
    cells, order = torch.sort(cell)                           # every cell lies in one brick: the keys are distinct
    face_off, n_faces = _face_offsets(ntri, t[order])
    keys = torch.empty(cells.numel() * 12, dtype=torch.int64, device=dev)
    d.cells, d.face_off, d.edge_keys, d.n_cells, d.n_faces = ptr(cells), ptr(face_off), ptr(keys), cells.numel(), n_faces
    call(prefix + "edges", d)
    edges = torch.unique(keys)                                # ascending; INT64_MAX (no vertex on that edge) comes last
    del keys
    if edges.numel() and int(edges[-1]) == torch.iinfo(torch.int64).max:
        edges = edges[:-1].contiguous()
    faces = torch.empty((n_faces, 3), dtype=torch.int64, device=dev)
    verts = torch.empty((edges.numel(), 3), dtype=torch.float32, device=dev)
    d.edges, d.faces, d.verts, d.n_edges = ptr(edges), ptr(faces), ptr(verts), edges.numel()
    mark("emit")
    call(prefix + "emit", d)
    mark("vertices")
    call(prefix + "vertices", d)
    mark(None)
    return verts, faces


def udf_marching_cubes_sparse(grid, _events=None):
    """MeshUDF marching cubes of a SparseUDFGrid (csrc/meshudf_sparse.hip) -> (verts [V, 3] fp32, faces [F, 3] int64),
    device tensors, unfiltered: the mesh `udf_marching_cubes(*grid.to_dense(), ...)` gives, in the same order (vertices
    ascending by global edge id, faces by ascending global cell index, then table order), without any N^3 array.  The
    cells with triangles and the unique edge ids are sorted with torch integer sorts over active cells and edges only.
    (`_events`: stage events -- classify, sort, emit, vertices -- for scripts/bench_meshudf_sparse.py.)"""
    if not isinstance(grid, SparseUDFGrid):
        raise ValueError("grid must be a SparseUDFGrid (udf_sparse_grid)")

    def desc(**fields):
        mean_thr, max_thr = thresholds(grid_spacing(grid.bound_min, grid.bound_max, grid.N))
        return _lib.MeshUDFSparse(mean_thr=float(mean_thr), max_thr=float(max_thr), **fields)
    return _mesh_sparse(grid, desc, "nudf_meshudf_sparse_", _events, check_nb=False)


# ---- level sets: the surface {F = level} of a signed or unsigned field (csrc/isosurface.hip) ----------------------------

def _check_level(level):
    if isinstance(level, (bool, str)) or not isinstance(level, (int, float, np.floating, np.integer)) \
            or not math.isfinite(level) or abs(level) > float(np.finfo(np.float32).max):
        raise ValueError(f"level {level!r} is not a finite real number (in fp32)")
    return float(np.float32(level))


def iso_marching_cubes(F, level, bound_min, bound_max, _events=None):
    """marching cubes of the level set {F = level} of a dense grid (csrc/isosurface.hip) -> (verts [V, 3] fp32,
    faces [F, 3] int64), device tensors.  F: [N, N, N] fp32 on one GPU, signed or not, on the grid
    linspace(bound_min, bound_max, N) per axis (x-major); `level` is rounded to fp32.  Corner c of a cell is `-` iff
    F_c < level; a cell with a NaN or infinite corner emits nothing.  One vertex per sign-change edge at the linear
    interpolation (the vertex set of any marching cubes); the triangulation of ambiguous cases (mc_tables.py: cells that
    agree on a shared face cut it the same way, so the mesh has no cracks), the winding (normals point to the `+` side)
    and the order (vertices by edge id 3 lin(lower end) + axis, faces by cell and table order) are this library's.
    Triangles of zero area occur where a node equals the level and are kept.  Empty inputs and fields with no crossing
    give empty outputs.  (`_events`: stage events -- classify, scan, emit, vertices -- for scripts/bench_isosurface.py.)"""
    if not isinstance(F, torch.Tensor):
        raise ValueError("F must be a torch tensor")
    if F.dtype != torch.float32:
        raise ValueError(f"F must be float32 (got {F.dtype})")
    if not F.is_cuda:
        raise ValueError(f"F must be on a GPU (got {F.device})")
    if F.dim() != 3 or not F.shape[0] == F.shape[1] == F.shape[2]:
        raise ValueError(f"F must be [N, N, N] (got {tuple(F.shape)})")
    level = _check_level(level)
    n, dev = F.shape[0], F.device
    if n == 0:
        return _empty_mesh(dev)
    _check_n(n)
    F = F.contiguous()
    axes = rb._grid_axes(bound_min, bound_max, n, dev).contiguous()
    return _mesh_dense(_lib.IsoSurface(F=ptr(F), axes=ptr(axes), N=n, level=level), "nudf_isosurface_", n, dev, _events)


def iso_selection_bounds(bound_min, bound_max, resolution, level, block, lipschitz):
    """(lo, hi) fp32: a block is selected iff the minimum of its coarse corners is <= lo and their maximum is >= hi, with
    lo = level + lipschitz r and hi = level - lipschitz r (level: rounded to fp32 first; r: half the diagonal of a block of
    `block` cells per axis), evaluated in float64 and rounded outward -- lo up, hi down -- to fp32"""
    n = int(resolution)
    ha = [(float(bound_max[a]) - float(bound_min[a])) / (n - 1) for a in range(3)]
    reach = float(lipschitz) * (0.5 * math.sqrt(sum((block * x) ** 2 for x in ha)))
    lv = float(np.float32(level))
    lo, hi = np.float32(lv + reach), np.float32(lv - reach)
    if float(lo) < lv + reach:
        lo = np.nextafter(lo, np.float32(np.inf))
    if float(hi) > lv - reach:
        hi = np.nextafter(hi, np.float32(-np.inf))
    return lo, hi


@torch.no_grad()
def iso_sparse_grid(query_func, resolution, level, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), block=8,
                    lipschitz=2.0, device=None, _events=None):
    """-> SparseFieldGrid: the values of `query_func(pts [P, 3]) -> [P]` (the callable extract_fields takes) on the
    blocks of `block`^3 cells that can contain a cell cut by {F = level} only; values are not clamped, signed fields are
    welcome.  `device` defaults to the current GPU.  The grid and its point coordinates are the dense path's.

    Selection: nb = ceil((N-1) / block) blocks per axis; the field is queried at the (nb+1)^3 coarse nodes
    min(b block, N-1); with cmin / cmax the minimum / maximum of a block's eight coarse corners and r half the block's
    diagonal, the block is selected iff cmin - lipschitz r <= level and cmax + lipschitz r >= level
    (`iso_selection_bounds`); a NaN corner makes it unselected.  Every node of a block lies within r of a corner and a
    cut cell needs a node below the level and one at or above it, so with |grad F| <= lipschitz no cut cell is lost.
    `lipschitz` is a safety parameter, not a measurement: a steeper field can lose cells.

    Every grid node of a selected block is queried exactly once (sorted unique node ids), so all brick copies of a shared
    node hold the same bits and block faces cannot crack.  No allocation is O(N^3); the coarse values and block_slot are
    O((N / block)^3).  (`_events`: stage events -- coarse, select, fine, bricks -- for scripts/bench_isosurface.py.)"""
    n = int(resolution)
    _check_sparse(n, block, lipschitz)
    _check_level(level)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    lo, hi = (torch.tensor(x, device=dev) for x in iso_selection_bounds(bound_min, bound_max, n, level, block, lipschitz))
    mark = _stage_marker(_events)

    def select(c):                                             # minimum and maximum propagate NaN: never selected
        return (_block_corners(c, torch.minimum) <= lo) & (_block_corners(c, torch.maximum) >= hi)
    geometry, coarse, nodes, vals, scatter = _select_and_query(query_func, select, None, n, block, bound_min, bound_max,
                                                               dev, mark)
    mark("bricks")
    F = scatter(vals, float("inf"))
    mark(None)
    return SparseFieldGrid(**geometry, F=F, coarse=coarse, n_queried=nodes.numel())


def iso_marching_cubes_sparse(grid, level, _events=None):
    """marching cubes of the level set {F = level} of a SparseFieldGrid (csrc/isosurface.hip) -> (verts [V, 3] fp32,
    faces [F, 3] int64), device tensors: the mesh `iso_marching_cubes` gives on a dense grid that holds the same values,
    in the same order, without any N^3 array.  `level` should be the one the grid was selected for (another level meshes
    only what the selected blocks hold of it).  (`_events`: stage events -- classify, sort, emit, vertices.)"""
    if not isinstance(grid, SparseFieldGrid):
        raise ValueError("grid must be a SparseFieldGrid (iso_sparse_grid)")
    level = _check_level(level)
    return _mesh_sparse(grid, lambda **fields: _lib.IsoSurfaceSparse(level=level, **fields), "nudf_isosurface_sparse_",
                        _events, check_nb=True)


def _to_host(verts, faces, scale_mat):
    """-> (vertices np.float32 [V, 3], faces np.int64 [F, 3]); `scale_mat` ([4, 4]) maps the vertices to world space as the
    runner does: v * S[0, 0] + S[:3, 3] (exp_runner_blending.py:794)"""
    v = verts.cpu().numpy()
    if scale_mat is not None:
        S = np.asarray(scale_mat, dtype=np.float64)
        v = (v * S[0, 0] + S[:3, 3][None]).astype(np.float32)
    return v, faces.cpu().numpy()


@torch.no_grad()
def extract_iso_mesh(query_func, resolution=256, level=0.0, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0),
                     scale_mat=None, sparse=False, block=8, lipschitz=2.0, min_component_faces=0, keep_largest=False,
                     device=None):
    """mesh of the level set {F = level} of `query_func(pts [P, 3]) -> [P]` on the GPU: what the reference's
    extract_geometry gets from PyMCubes for the {udf < t} shell (Runner.validate_mesh), and the zero set of a signed
    field (SDFNetwork, udf_type='sdf') at level 0.  Grid query on the device (the slabs of extract_fields) ->
    iso_marching_cubes; with sparse=True, iso_sparse_grid(block, lipschitz) -> iso_marching_cubes_sparse: only the blocks
    that can hold a cut cell are queried and meshed, resolutions up to 4096, the same mesh as long as the field is no
    steeper than `lipschitz`.  Components with fewer than min_component_faces faces are dropped, or with keep_largest
    all but the largest (meshclean.filter_components).  Triangles of zero area are kept.  `scale_mat` maps the vertices
    to world space as the runner does: v * S[0, 0] + S[:3, 3].  `device` defaults to the current GPU.
    -> (vertices np.float32 [V, 3], faces np.int64 [F, 3]).  Raises RuntimeError when the field does not cross the level."""
    n = int(resolution)
    level = _check_level(level)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if sparse:
        verts, faces = iso_marching_cubes_sparse(iso_sparse_grid(query_func, n, level, bound_min, bound_max, block,
                                                                 lipschitz, dev), level)
    else:
        _check_n(n)
        F = rb._grid_query_device(bound_min, bound_max, n, query_func, dev, 1)
        verts, faces = iso_marching_cubes(F, level, bound_min, bound_max)
        del F
    if faces.shape[0] and (min_component_faces > 0 or keep_largest):
        verts, faces = meshclean.filter_components(verts, faces, min_component_faces, keep_largest)
    if faces.shape[0] == 0:
        raise RuntimeError(f"no surface found: the field does not cross the level {level} on the grid")
    return _to_host(verts, faces, scale_mat)


def filter_mesh(verts, faces, vertex_udf, max_udf):
    """the reference's clean-up (extract_mesh.py:205-222) on device tensors, in this order: drop every face whose
    largest vertex UDF is >= max_udf, faces of zero area (fp32 cross product exactly 0) and repeated faces (same sorted
    vertex triple; the first one stays), then the vertices no face references (the others keep their order).
    -> (verts [V', 3], faces [F', 3] int64 into them)"""
    vu = vertex_udf.reshape(-1)
    faces = faces[vu[faces].amax(1) < max_udf] if faces.numel() else faces
    if faces.numel():
        v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
        faces = faces[(torch.linalg.cross(v1 - v0, v2 - v0) != 0).any(1)]
    if faces.numel():
        f = faces.shape[0]
        _, inv = torch.unique(faces.sort(1).values, dim=0, return_inverse=True)
        order = torch.arange(f, device=faces.device)
        first = torch.full((int(inv.max()) + 1,), f, dtype=torch.int64, device=faces.device)
        first.scatter_reduce_(0, inv, order, "amin")
        faces = faces[first[inv] == order]
    return compact_mesh(verts, faces)


@torch.no_grad()
def _query_udf(udf_network, pts):
    chunk = rb.GRID_CHUNK_POINTS
    return torch.cat([udf_network.udf(pts[s:s + chunk])[:, 0] for s in range(0, pts.shape[0], chunk)])


def extract_udf_mesh(udf_network, resolution=256, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0),
                     dist_threshold_ratio=1.0, scale_mat=None, fill_holes=False, smooth_borders=False,
                     min_component_faces=0, keep_largest=False, sparse=False, block=8, lipschitz=2.0, orient=False,
                     outward_from=None, color_from=None, simplify_cell=None, simplify_max_error=None, smooth=None,
                     denoise=False, subdivide_max_edge=None, subdivide=None, close_holes=None,
                     close_holes_perimeter=None, close_holes_check=False, drop_self_intersections=False,
                     remesh_edge=None, remesh_iterations=5, texture_from=None, texture_density=None, texture_size=None):
    """open-surface mesh of `udf_network`'s zero level (the reference's get_mesh_udf_fast, without its differentiable
    refinement): udf_grid -> udf_marching_cubes -> filter_mesh with the network's UDF at the vertices and
    max_udf = dist_threshold_ratio * h.  The clean-up the reference takes from trimesh is off by default and follows in
    its order when asked for (neuraludf_amd.meshclean): fill_holes (holes of 3 and 4 edges), smooth_borders (5 steps,
    lambda 0.3; with close_holes = n the border loops of up to n <= 64 edges, and of a perimeter of at most
    close_holes_perimeter in the coordinates of the box when that is given, are closed between the two with their
    minimum-area triangulation: meshclean.close_holes; with close_holes_check=True the patches that pass through the
    surface or lie folded onto it are taken back: meshclean.close_holes_checked), then the components with fewer than min_component_faces faces are
    dropped, or with keep_largest all but the largest.  With `scale_mat` ([4, 4], the dataset's scale_mats_np[0]) the
    vertices are mapped to world space as the runner does: v * S[0, 0] + S[:3, 3] (exp_runner_blending.py:794).
    With sparse=True, udf_sparse_grid(block,
    lipschitz) -> udf_marching_cubes_sparse replace the dense grid and mesher: only the blocks near the surface are
    queried and meshed, resolutions up to 4096 are possible, and the mesh is the dense one as long as the field is no
    steeper than `lipschitz` (a steeper field can lose cells); everything after the mesher is unchanged.
    With simplify_cell = c, in the coordinates of the box, the mesh is simplified after the component filter by vertex
    clustering on a grid of edge c with quadric placement (meshclean.simplify_mesh): the orientation and the colouring
    see the final mesh.  With simplify_max_error = e instead, in the same coordinates, the grid is searched for
    (meshclean.simplify_to_error): the result's measured two-sided deviation from the unsimplified mesh is at most e.
    With denoise=True (or a dict of meshclean.denoise_mesh's arguments) and with smooth = an iteration count (or a dict of
    meshclean.smooth_mesh's arguments) the mesher's grid noise is filtered after the component filter and before the
    simplification, which would freeze it into larger triangles: the bilateral normal filter first, then the Taubin
    smoothing, when both are given.
    With remesh_edge = L, in the coordinates of the box, the mesh is remeshed isotropically after the simplification and
    before the subdivision, in remesh_iterations iterations, towards well-shaped triangles with edges of length L, its
    vertices kept on the surface as it was before the step (meshclean.remesh_isotropic).
    With subdivide_max_edge = h, in the coordinates of the box, the edges longer than h are split at their midpoints after
    the simplification until none is left (meshclean.subdivide_to_edge; the surface does not change), and with subdivide =
    a level count (or a dict of meshclean.subdivide_mesh's arguments) the mesh is then subdivided uniformly, by Loop's
    scheme unless the dict says otherwise: the orientation and the colouring see the denser mesh, so that color_from takes
    one colour sample per vertex of it.
    With drop_self_intersections=True the faces that pass through each other or lie folded onto each other are dropped
    after the subdivision (meshclean.drop_self_intersections: every step before it moves or merges vertices and can fold
    the surface over itself), with the vertices they leave unused.
    With orient=True the faces of every orientable component are wound consistently as the last step
    (meshclean.orient_faces; after the hole filler, which adds faces): the mesher decides its winding cell by cell, and
    about two faces in five of its output are wound against their neighbours.  `outward_from` (x, y, z), in the
    coordinates of the box, i.e. before `scale_mat`, picks the winding that turns away from that point and implies
    orient=True.  Vertices, face order and counts do not change.
    `color_from` = (world_mats [n, 4, 4], images [n, H, W, 3] uint8 or float32 on the GPU), in the coordinates of the box
    (meshrender.dataset_views gives the pair of a training source), colours the vertices from the images as the last
    step, weighted by the vertex normals of the mesh as it then is (meshrender.color_vertices), and adds a third value.
    `texture_from` = the same pair, in place of color_from (giving both is a ValueError), bakes a texture as the last
    step instead: an atlas with one chart per face (meshrender.texture_atlas with texture_density texels per unit length
    of the box, or the largest density whose atlas is at most texture_size texels wide; 4096 when neither is given) is
    coloured texel by texel as color_from colours vertices (meshrender.bake_texture), and the texels no view sees take
    the mix of the vertex colours, which are computed for that purpose only.  The colour resolution no longer hangs on
    the vertex count: simplify first.  It adds two values, uv np.float32 [F, 3, 2], normalised ((u + 0.5) / W, (v + 0.5)
    / H of the texel-centre coordinates, v downwards as the texture's rows run: write_obj flips it), and texture np.uint8
    [H, W, 3].
    -> (vertices np.float32 [V, 3], faces np.int64 [F, 3]), with color_from also colors np.float32 [V, 3], with
    texture_from also uv and texture.  Raises RuntimeError when no surface is found."""
    if texture_from is not None and color_from is not None:
        raise ValueError("texture_from and color_from exclude each other")
    if texture_from is None and (texture_density is not None or texture_size is not None):
        raise ValueError("texture_density and texture_size need texture_from")
    if texture_density is not None and texture_size is not None:
        raise ValueError("texture_density and texture_size exclude each other")
    n = int(resolution)
    if sparse:
        verts, faces = udf_marching_cubes_sparse(udf_sparse_grid(udf_network, n, bound_min, bound_max, block, lipschitz))
    else:
        U, G = udf_grid(udf_network, n, bound_min, bound_max)
        verts, faces = udf_marching_cubes(U, G, bound_min, bound_max)
        del U, G
    if faces.shape[0]:
        h = grid_spacing(bound_min, bound_max, n)
        verts, faces = filter_mesh(verts, faces, _query_udf(udf_network, verts), dist_threshold_ratio * h)
    if fill_holes:
        faces, _ = meshclean.fill_holes(verts, faces)
    if close_holes is not None:
        if close_holes_check:
            faces = meshclean.close_holes_checked(verts, faces, close_holes, close_holes_perimeter)[0].faces
        else:
            faces = meshclean.close_holes(verts, faces, close_holes, close_holes_perimeter).faces
    elif close_holes_perimeter is not None:
        raise ValueError("close_holes_perimeter needs close_holes")
    elif close_holes_check:
        raise ValueError("close_holes_check needs close_holes")
    if smooth_borders:
        verts = meshclean.smooth_borders(verts, faces)
    if min_component_faces > 0 or keep_largest:
        verts, faces = meshclean.filter_components(verts, faces, min_component_faces, keep_largest)
    if simplify_cell is not None and simplify_max_error is not None:
        raise ValueError("simplify_cell and simplify_max_error exclude each other")
    if denoise:
        verts = meshclean.denoise_mesh(verts, faces, **(denoise if isinstance(denoise, dict) else {}))[0]
    if smooth is not None:
        verts = meshclean.smooth_mesh(verts, faces, **(smooth if isinstance(smooth, dict) else dict(iterations=smooth)))
    if simplify_cell is not None:
        verts, faces = meshclean.simplify_mesh(verts, faces, simplify_cell)[:2]
    if simplify_max_error is not None and faces.shape[0]:
        verts, faces = meshclean.simplify_to_error(verts, faces, simplify_max_error)[0][:2]
    if remesh_edge is not None:
        verts, faces = meshclean.remesh_isotropic(verts, faces, remesh_edge, remesh_iterations)[:2]
    if subdivide_max_edge is not None:
        verts, faces = meshclean.subdivide_to_edge(verts, faces, subdivide_max_edge)[:2]
    if subdivide is not None:
        verts, faces = meshclean.subdivide_mesh(
            verts, faces, **(subdivide if isinstance(subdivide, dict) else dict(levels=subdivide)))[:2]
    if drop_self_intersections:
        verts, faces, _ = meshclean.drop_self_intersections(verts, faces)
    if orient or outward_from is not None:
        faces = meshclean.orient_faces(verts, faces, outward_from).faces
    if faces.shape[0] == 0:
        raise RuntimeError("no surface found: no grid cell of the UDF is close enough to its zero level")
    if color_from is not None:
        mats, images = color_from
        colors, _ = meshrender.color_vertices(verts, faces, mats, images.to(verts.device),
                                              normals=meshclean.vertex_normals(verts, faces, torch.float64))
        return _to_host(verts, faces, scale_mat) + (colors.cpu().numpy(),)
    if texture_from is not None:
        mats, images = texture_from
        uv, texture = _bake(verts, faces, mats, images.to(verts.device), texture_density,
                            4096 if texture_density is None and texture_size is None else texture_size)[:2]
        return _to_host(verts, faces, scale_mat) + (uv, texture)
    return _to_host(verts, faces, scale_mat)


def _bake(verts, faces, mats, images, density, size):
    """atlas, vertex colours as the fallback, bake -> (uv np.float32 [F, 3, 2] normalised, texture np.uint8 [H, W, 3],
    Atlas, Texture)"""
    normals = meshclean.vertex_normals(verts, faces, torch.float64)
    atlas = meshrender.texture_atlas(verts, faces, density=density, size=size)
    fallback, _ = meshrender.color_vertices(verts, faces, mats, images, normals=normals)
    tex = meshrender.bake_texture(verts, faces, atlas, mats, images, normals=normals, fallback=fallback)
    wh = torch.tensor([atlas.W, atlas.H], dtype=torch.float64, device=verts.device)
    uv = ((atlas.uv + 0.5) / wh).float().cpu().numpy()
    texture = _uchar_colors(tex.colors.cpu().numpy()).reshape(atlas.H, atlas.W, 3)
    return uv, texture, atlas, tex


def _uchar_colors(colors):
    """[N, 3] floats in [0, 1], rounded to the nearest of 0..255, or uint8 -> uint8 [N, 3]"""
    c = np.asarray(colors).reshape(-1, 3)
    if c.dtype != np.uint8:
        c = np.rint(np.clip(np.asarray(c, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
    return c


def write_ply(path, vertices, faces, normals=None, colors=None):
    """binary little-endian PLY: float x, y, z per vertex, followed by float nx, ny, nz when `normals` [V, 3] are given and
    by uchar red, green, blue when `colors` [V, 3] are (floats in [0, 1], rounded as write_points_ply does, or uint8); a
    uchar count and int32 indices per face"""
    v = np.asarray(vertices, dtype="<f4").reshape(-1, 3)
    fields, cols, props = [("p", "<f4", (3,))], dict(p=v), "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        cols["n"] = np.asarray(normals, dtype="<f4").reshape(-1, 3)
        if len(cols["n"]) != len(v):
            raise ValueError("vertices and normals differ in length")
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        cols["c"] = _uchar_colors(colors)
        if len(cols["c"]) != len(v):
            raise ValueError("vertices and colors differ in length")
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    vrec = np.empty(len(v), dtype=fields)                  # packed: without colours, the floats one after the other
    for name, col in cols.items():
        vrec[name] = col
    f = np.asarray(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("face index out of range")
    rec = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"], rec["v"] = 3, f
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), props, len(f)))
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(rec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def write_obj(path, vertices, faces, uv, texture):
    """a textured mesh as Wavefront OBJ: NAME.obj with `v` lines, three `vt` lines per face and `f a/ta b/tb c/tc` lines,
    NAME.mtl with one material whose map_Kd is NAME.png, and the texture as NAME.png, all next to each other (`path` is
    NAME.obj).  uv [F, 3, 2]: normalised, ((i + 0.5) / W, (j + 0.5) / H) for the texel-centre coordinates (i, j) of
    meshrender.Atlas.uv, v downwards as the texture's rows run; OBJ's v runs upwards, so vt = (u, 1 - v).  texture
    [H, W, 3]: uint8, or floats in [0, 1], rounded as write_ply rounds colours.  Numbers are written with the fewest digits
    that read back to the same float32 or float64; the atlas's UVs are odd multiples of 1 / 2 W and 1 / 2 H, for which 1 -
    v is exact."""
    import os
    from PIL import Image
    path = str(path)
    stem = path[:-4] if path.lower().endswith(".obj") else path
    name = os.path.basename(stem)
    v, f = np.asarray(vertices), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v = v.reshape(-1, 3)
    uv = np.asarray(uv)
    if uv.shape != (len(f), 3, 2):
        raise ValueError(f"uv must be [{len(f)}, 3, 2] (got {uv.shape})")
    tex = np.asarray(texture)
    if tex.ndim != 3 or tex.shape[2] != 3:
        raise ValueError(f"texture must be [H, W, 3] (got {tex.shape})")
    tex = _uchar_colors(tex).reshape(tex.shape)
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %s %s %s" % tuple(p) for p in v]                              # str of a numpy float: the shortest that reads back
    lines += ["vt %s %s" % (t[0], 1 - t[1]) for t in uv.reshape(-1, 2)]
    lines += ["f %d/%d %d/%d %d/%d" % (a + 1, 3 * i + 1, b + 1, 3 * i + 2, c + 1, 3 * i + 3) for i, (a, b, c) in enumerate(f)]
    with open(stem + ".obj", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    Image.fromarray(tex).save(stem + ".png")


def read_obj(path):
    """what write_obj writes -> (vertices np.float64 [V, 3], faces np.int64 [F, 3], uv np.float64 [F, 3, 2] with v
    downwards again (1 - vt.v), texture np.uint8 [H, W, 3] or None): `v`, `vt`, triangular `f v/vt` (a normal index
    after a second slash is ignored), and the map_Kd of the mtllib, both resolved next to the file.  Not a general OBJ
    reader: anything else on a line that it needs is a ValueError, other lines are skipped."""
    import os
    from PIL import Image
    path = str(path)
    v, vt, fv, ft, mtl = [], [], [], [], None
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            try:
                if w[0] == "v":
                    v.append([float(x) for x in w[1:4]])
                elif w[0] == "vt":
                    vt.append([float(x) for x in w[1:3]])
                elif w[0] == "f":
                    if len(w) != 4:
                        raise ValueError("not a triangle")
                    idx = [x.split("/") for x in w[1:]]
                    fv.append([int(x[0]) - 1 for x in idx])
                    ft.append([int(x[1]) - 1 for x in idx])
                elif w[0] == "mtllib":
                    mtl = line.split(None, 1)[1].strip()
            except (ValueError, IndexError) as e:
                raise ValueError(f"{path}:{n}: {line.strip()!r}: {e}") from None
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    vt = np.asarray(vt, dtype=np.float64).reshape(-1, 2)
    fv, ft = np.asarray(fv, dtype=np.int64).reshape(-1, 3), np.asarray(ft, dtype=np.int64).reshape(-1, 3)
    if fv.size and (fv.min() < 0 or fv.max() >= len(v) or ft.min() < 0 or ft.max() >= len(vt)):
        raise ValueError(f"{path}: a face index is out of range")
    uv = vt[ft]
    uv[..., 1] = 1.0 - uv[..., 1]
    texture, here = None, os.path.dirname(path)
    if mtl is not None and os.path.exists(os.path.join(here, mtl)):
        with open(os.path.join(here, mtl)) as fh:
            for line in fh:
                w = line.split(None, 1)
                if len(w) == 2 and w[0] == "map_Kd":
                    texture = np.ascontiguousarray(np.asarray(Image.open(os.path.join(here, w[1].strip())).convert("RGB"),
                                                              dtype=np.uint8))
    return v, fv, uv, texture


def _ply_header(fh):
    """-> (format, [(element name, count, [(property name, type) or (name, (count type, item type))])])"""
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header has no end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            break
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("PLY property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"unsupported PLY format {fmt}")
    return fmt, elements


def _ply_binary_element(buf, pos, count, props, endian):
    """-> (structured array or None, {list name: [count, k] index array}, new pos) of one binary element"""
    lists = [p for p in props if isinstance(p[1], tuple)]
    if not lists:
        dt = np.dtype([(n, endian + t) for n, t in props])
        return np.frombuffer(buf, dt, count, pos), {}, pos + dt.itemsize * count
    # a list element (faces): every list is taken to have the length of the first row's, then checked
    k, off = {}, pos
    for n, t in props:
        if isinstance(t, tuple):
            k[n] = int(np.frombuffer(buf, endian + t[0], 1, off)[0]) if count else 0
            off += np.dtype(t[0]).itemsize + k[n] * np.dtype(t[1]).itemsize
        else:
            off += np.dtype(t).itemsize
    fields = []
    for n, t in props:
        if isinstance(t, tuple):
            fields += [(n + "__n", endian + t[0]), (n, endian + t[1], (k[n],))]
        else:
            fields.append((n, endian + t))
    dt = np.dtype(fields)
    rec = np.frombuffer(buf, dt, count, pos) if len(buf) - pos >= dt.itemsize * count else None
    if rec is None or any((rec[n + "__n"] != k[n]).any() for n in k):
        raise ValueError("PLY lists of varying length (polygons that are not triangles) are not supported")
    return rec, {n: rec[n] for n in k}, pos + dt.itemsize * count


def read_ply(path, with_normals=False, with_colors=False):
    """vertices and triangles of a PLY file -> (vertices float64 [V, 3], faces int64 [F, 3] or None when the file has no
    face element); with_normals=True adds a third value, the vertices' nx / ny / nz as float64 [V, 3] or None when the
    file has none; with_colors=True adds a last value, the vertices' red / green / blue as they are stored (uint8 [V, 3]
    for uchar properties) or None when the file has none.  ASCII, binary little- and big-endian; vertex elements may carry further properties (normals, colours,
    double coordinates); faces are a list property (vertex_indices or vertex_index) of any integer types, triangles only."""
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh)
        body = fh.read()
    verts, faces, normals, colors = None, None, None, None
    rgb = ("red", "green", "blue")
    if fmt == "ascii":
        lines = iter(body.decode("ascii").split("\n"))
        for name, count, props in elements:
            rows = []
            for _ in range(count):
                line = next(lines).split()
                while not line:
                    line = next(lines).split()
                rows.append(line)
            if name == "vertex":
                cols = [[n for n, _ in props].index(a) for a in "xyz"]
                verts = np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).reshape(-1, 3)
                if all(a in [n for n, _ in props] for a in ("nx", "ny", "nz")):
                    cols = [[n for n, _ in props].index(a) for a in ("nx", "ny", "nz")]
                    normals = np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).reshape(-1, 3)
                if all(a in [n for n, _ in props] for a in rgb):
                    cols = [[n for n, _ in props].index(a) for a in rgb]
                    kind = np.result_type(*[np.dtype(dict(props)[a]) for a in rgb])
                    colors = np.array([[float(r[c]) for c in cols] for r in rows]).reshape(-1, 3).astype(kind)
            elif name == "face":
                if any(int(r[0]) != 3 for r in rows):
                    raise ValueError("only triangle faces are supported")
                faces = np.array([[int(v) for v in r[1:4]] for r in rows], dtype=np.int64).reshape(-1, 3)
    else:
        endian = "<" if fmt == "binary_little_endian" else ">"
        pos = 0
        for name, count, props in elements:
            rec, lists, pos = _ply_binary_element(body, pos, count, props, endian)
            if name == "vertex":
                verts = np.stack([rec[a].astype(np.float64) for a in "xyz"], -1).reshape(-1, 3)
                if all(a in rec.dtype.names for a in ("nx", "ny", "nz")):
                    normals = np.stack([rec[a].astype(np.float64) for a in ("nx", "ny", "nz")], -1).reshape(-1, 3)
                if all(a in rec.dtype.names for a in rgb):
                    colors = np.stack([rec[a] for a in rgb], -1).reshape(-1, 3)
            elif name == "face":
                key = "vertex_indices" if "vertex_indices" in lists else "vertex_index"
                if key not in lists:
                    raise ValueError("PLY face element has no vertex_indices list")
                faces = np.asarray(lists[key], dtype=np.int64).reshape(-1, 3)
    if verts is None:
        raise ValueError("PLY file has no vertex element")
    if faces is not None and faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("face index out of range")
    return (verts, faces) + ((normals,) if with_normals else ()) + ((colors,) if with_colors else ())


def write_points_ply(path, points, colors):
    """binary little-endian PLY point cloud: double x, y, z and uchar red, green, blue per point (colors: [N, 3] floats in
    [0, 1], rounded to the nearest of 0..255, or uint8)"""
    p = np.asarray(points, dtype="<f8").reshape(-1, 3)
    c = np.asarray(colors).reshape(-1, 3)
    if len(c) != len(p):
        raise ValueError("points and colors differ in length")
    c = _uchar_colors(c)
    rec = np.empty(len(p), dtype=[("p", "<f8", (3,)), ("c", "u1", (3,))])
    rec["p"], rec["c"] = p, c
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
            "property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(p))
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(rec.tobytes())


def load_dtu_images(dataset_dir, scan):
    """the source images of a DTU scan, next to the masks load_dtu_views reads: <dataset_dir>/scan<scan>/image/*.png in
    sorted order -> np.uint8 [n, H, W, 3], red, green, blue"""
    import glob
    import os
    from PIL import Image
    root = os.path.join(str(dataset_dir), f"scan{scan}")
    files = sorted(glob.glob(os.path.join(root, "image", "*.png")))
    if not files:
        raise FileNotFoundError(f"no image/*.png under {root}")
    return np.stack([np.ascontiguousarray(np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8)) for f in files])


def _write_renders(out_dir, verts, faces, normals, world_mats, H, W, view_chunk=8, textured=None):
    """normal_<i>.png (world-space normals, (n + 1) / 2 as 8-bit red, green, blue; black where nothing was drawn) and
    depth_<i>.npy (float32 [H, W], +inf where nothing was drawn) of the mesh from every view; with textured = (Atlas,
    Texture) also texture_<i>.png, the mesh drawn with its texture (meshrender.shade_textured; black where nothing was
    drawn)"""
    import os
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    for s in range(0, len(world_mats), view_chunk):
        r = meshrender.rasterize(verts, faces, world_mats[s:s + view_chunk], H, W, view_chunk)
        nm = meshrender.normal_map(r, faces, normals)
        img = torch.where((r.face >= 0)[..., None], (nm + 1.0) * 0.5, torch.zeros_like(nm))
        img = (img.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).cpu().numpy()
        depth = r.depth.cpu().numpy()
        if textured is not None:
            shaded = meshrender.shade_textured(r, *textured)
            shaded = (shaded.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).cpu().numpy()
        for k in range(len(depth)):
            if textured is not None:
                Image.fromarray(shaded[k]).save(os.path.join(out_dir, f"texture_{s + k}.png"))
            Image.fromarray(img[k]).save(os.path.join(out_dir, f"normal_{s + k}.png"))
            np.save(os.path.join(out_dir, f"depth_{s + k}.npy"), depth[k])


def main(argv=None):
    """python -m neuraludf_amd.meshing IN.ply OUT.ply ...: the clean-up steps on a mesh file, in the reference's order
    (holes, borders, components, then the DTU mask and visual-hull cleaning), then the denoising and the smoothing (the
    file's colours pass through them untouched), the simplification, the isotropic remeshing (--remesh; the file's colours
    are carried from the closest points of the mesh before it), the subdivision (edges above --max-edge first, then
    --subdivide levels; the file's colours go through the weights of the positions), the orientation of the faces, the
    vertex normals and, last of all, the vertex colours and the renders from the scan's cameras; `python -m
    neuraludf_amd.evaluation` scores the result"""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m neuraludf_amd.meshing", description=main.__doc__)
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--fill-holes", action="store_true")
    ap.add_argument("--smooth-borders", action="store_true")
    ap.add_argument("--border-loops", action="store_true", help="print the table of the input's border loops; changes nothing")
    ap.add_argument("--close-holes", type=int, metavar="N",
                    help="after --fill-holes, close the border loops of up to N <= 64 edges (minimum-area triangulation)")
    ap.add_argument("--close-holes-perimeter", type=float, metavar="P", help="with --close-holes: leave longer loops open")
    ap.add_argument("--close-holes-check", action="store_true",
                    help="with --close-holes: take back the patches that pass through the surface (close_holes_checked)")
    ap.add_argument("--drop-self-intersections", action="store_true",
                    help="before the orientation, drop the faces that pass through or lie folded onto each other")
    grp = ap.add_mutually_exclusive_group()
    grp.add_argument("--min-faces", type=int, default=0, help="drop the components with fewer faces")
    grp.add_argument("--keep-largest", action="store_true", help="keep the largest component only")
    ap.add_argument("--dtu-dir", help="DTU dataset directory (scan<N>/cameras.npz, scan<N>/mask/*.png)")
    ap.add_argument("--scan", type=int)
    ap.add_argument("--mask-dilated-size", type=int, default=11)
    ap.add_argument("--minimal-vis", type=int, default=2)
    grp = ap.add_mutually_exclusive_group()
    grp.add_argument("--simplify", type=float, metavar="CELL",
                     help="simplify by vertex clustering on a grid of this edge length, with quadric placement")
    grp.add_argument("--simplify-to", type=int, metavar="FACES", help="simplify to at most this many faces")
    grp.add_argument("--simplify-max-error", type=float, metavar="E",
                     help="simplify on the coarsest grid found whose measured two-sided deviation from the input is <= E")
    ap.add_argument("--denoise", action="store_true",
                    help="bilateral normal filter and vertex update (denoise_mesh), before --smooth and the simplification")
    ap.add_argument("--sigma-s", type=float, default=0.35, metavar="S", help="normal term of --denoise")
    ap.add_argument("--smooth", type=int, metavar="N", help="N rounds of Taubin smoothing (smooth_mesh)")
    ap.add_argument("--smooth-weights", choices=("uniform", "cotangent"), default="uniform")
    ap.add_argument("--free-boundary", action="store_true", help="let border vertices move under --smooth and --denoise")
    ap.add_argument("--remesh", type=float, metavar="L",
                    help="after the simplification, remesh isotropically towards edges of length L (remesh_isotropic)")
    ap.add_argument("--remesh-iterations", type=int, default=5, metavar="N", help="iterations of --remesh")
    ap.add_argument("--max-edge", type=float, metavar="H",
                    help="after the simplification, split edges at their midpoints until none is longer than H")
    ap.add_argument("--subdivide", type=int, metavar="N", help="N levels of uniform subdivision (subdivide_mesh)")
    ap.add_argument("--subdivide-scheme", choices=("loop", "midpoint"), default="loop")
    ap.add_argument("--orient", action="store_true", help="wind the faces of every orientable component consistently")
    ap.add_argument("--outward-from", type=float, nargs=3, metavar=("X", "Y", "Z"),
                    help="wind every component away from this point (implies --orient)")
    ap.add_argument("--normals", action="store_true", help="write angle-weighted vertex normals (nx, ny, nz)")
    ap.add_argument("--colour", action="store_true",
                    help="colour the vertices from scan<N>/image/*.png (needs --dtu-dir and --scan; red, green, blue)")
    ap.add_argument("--render", metavar="DIR",
                    help="write normal_<i>.png and depth_<i>.npy of the mesh from every camera of the scan into DIR")
    ap.add_argument("--texture", metavar="OUT.obj",
                    help="bake a texture atlas from scan<N>/image/*.png and write OUT.obj, OUT.mtl and OUT.png (needs "
                         "--dtu-dir and --scan); --render then also writes texture_<i>.png")
    grp = ap.add_mutually_exclusive_group()
    grp.add_argument("--texture-size", type=int, metavar="N",
                     help="the largest atlas width: the densest atlas that fits is used (default 4096)")
    grp.add_argument("--texture-density", type=float, metavar="D", help="texels per unit length instead")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.texture and a.dtu_dir is None:
        ap.error("--texture needs --dtu-dir and --scan")
    if (a.texture_size is not None or a.texture_density is not None) and not a.texture:
        ap.error("--texture-size and --texture-density need --texture")
    if (a.dtu_dir is None) != (a.scan is None):
        ap.error("--dtu-dir and --scan go together")
    if (a.colour or a.render) and a.dtu_dir is None:
        ap.error("--colour and --render need --dtu-dir and --scan")
    if a.close_holes_perimeter is not None and a.close_holes is None:
        ap.error("--close-holes-perimeter needs --close-holes")
    if a.close_holes_check and a.close_holes is None:
        ap.error("--close-holes-check needs --close-holes")
    v, f, file_colors = read_ply(a.input, with_colors=True)
    if f is None:
        ap.error(f"{a.input} has no faces")
    dev = torch.device(a.device)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    n0 = (verts.shape[0], faces.shape[0])
    if a.fill_holes:
        faces, n = meshclean.fill_holes(verts, faces)
        print(f"fill_holes: {n} holes closed")
    if a.border_loops:
        loops = meshclean.border_loops(verts, faces)
        n_edges = (loops.loop_off[1:] - loops.loop_off[:-1]).tolist()
        print(f"border_loops: {len(n_edges)} loops")
        for i, (c, n, p) in enumerate(zip(loops.closed.tolist(), n_edges, loops.perimeter.tolist())):
            print(f"  loop {i}: {'closed' if c else 'open'}, {n} edges, perimeter {p:.6g}")
    if a.close_holes is not None:
        if a.close_holes_check:
            closed, back = meshclean.close_holes_checked(verts, faces, a.close_holes, a.close_holes_perimeter)
            print(f"close_holes_check: {back.numel()} patches taken back (loops {back.tolist()})")
        else:
            closed = meshclean.close_holes(verts, faces, a.close_holes, a.close_holes_perimeter)
        faces = closed.faces
        tally = torch.bincount(closed.status.long(), minlength=len(meshclean.HOLE_STATUS_NAMES)).tolist()
        detail = ", ".join(f"{meshclean.HOLE_STATUS_NAMES[k]} {c}" for k, c in enumerate(tally) if c)
        print(f"close_holes: {tally[meshclean.HOLE_FILLED]} of {closed.status.numel()} loops closed ({detail or 'no border'})")
    if a.smooth_borders:
        verts = meshclean.smooth_borders(verts, faces)
    if a.min_faces > 0 or a.keep_largest:
        verts, faces = meshclean.filter_components(verts, faces, a.min_faces, a.keep_largest)
    if a.dtu_dir is not None:
        mats, masks = load_dtu_views(a.dtu_dir, a.scan)
        verts, faces = meshclean.clean_dtu_mesh(verts, faces, mats, torch.from_numpy(masks).to(dev),
                                                a.mask_dilated_size, a.minimal_vis)
    carried = None                                           # mean colours of the clusters, as the file stores colours
    if a.denoise or a.smooth is not None:
        boundary = "free" if a.free_boundary else "fixed"
        if a.denoise:
            verts = meshclean.denoise_mesh(verts, faces, sigma_s=a.sigma_s, boundary=boundary)[0]
        if a.smooth is not None:
            verts = meshclean.smooth_mesh(verts, faces, a.smooth, weights=a.smooth_weights, boundary=boundary)
        if file_colors is not None and not a.colour and len(file_colors) == verts.shape[0]:
            carried = file_colors                            # the filters move vertices, they neither add nor drop any
    if a.simplify is not None or a.simplify_to is not None or a.simplify_max_error is not None:
        attrs = carried = None
        if file_colors is not None and not a.colour:         # the file's colours travel as attributes unless --colour
            if len(file_colors) == verts.shape[0]:           # the clean-up only ever drops vertices
                attrs = torch.from_numpy(np.asarray(file_colors, dtype=np.float64)).to(dev)
            else:
                print("simplify: the clean-up dropped vertices, the file's colours are not carried")
        if a.simplify is not None:
            info = {}
            s = meshclean.simplify_mesh(verts, faces, a.simplify, attributes=attrs, _info=info)
            print(f"simplify: {info['clusters']} clusters, {info['fallbacks']} of {s.verts.shape[0]} vertices at the mean")
        elif a.simplify_to is not None:
            s = meshclean.simplify_to_faces(verts, faces, a.simplify_to, attributes=attrs)
        else:
            s, dev_ = meshclean.simplify_to_error(verts, faces, a.simplify_max_error, attributes=attrs)
            print(f"simplify: deviation hausdorff {dev_['hausdorff']} (input to result max {dev_['a_to_b']['max']}, "
                  f"result to input max {dev_['b_to_a']['max']}) <= {a.simplify_max_error}")
        verts, faces = s.verts, s.faces
        if attrs is not None:
            carried = s.attributes.cpu().numpy()
            if file_colors.dtype == np.uint8:                # a mean of 0..255 values is one
                carried = np.rint(carried).astype(np.uint8)
    simplified = a.simplify is not None or a.simplify_to is not None or a.simplify_max_error is not None
    if a.remesh is not None:
        attrs = None
        if carried is not None:                              # colours that came through the steps above
            attrs = torch.from_numpy(np.asarray(carried, dtype=np.float64)).to(dev)
        elif file_colors is not None and not a.colour and len(file_colors) == verts.shape[0] and not simplified:
            attrs = torch.from_numpy(np.asarray(file_colors, dtype=np.float64)).to(dev)
        r = meshclean.remesh_isotropic(verts, faces, a.remesh, a.remesh_iterations, attributes=attrs)
        print(f"remesh: split {list(r.split)}, collapsed {list(r.collapsed)}, flipped {list(r.flipped)}")
        verts, faces, carried = r.verts, r.faces, None
        if r.attributes is not None:
            carried = r.attributes.cpu().numpy()
            if file_colors.dtype == np.uint8:                # a convex combination of 0..255 values is one
                carried = np.rint(np.clip(carried, 0.0, 255.0)).astype(np.uint8)
    if a.max_edge is not None or a.subdivide is not None:
        attrs = None
        if carried is not None:                              # colours that came through the steps above
            attrs = torch.from_numpy(np.asarray(carried, dtype=np.float64)).to(dev)
        elif (file_colors is not None and not a.colour and len(file_colors) == verts.shape[0]
              and not simplified and a.remesh is None):
            attrs = torch.from_numpy(np.asarray(file_colors, dtype=np.float64)).to(dev)
        if a.max_edge is not None:
            s = meshclean.subdivide_to_edge(verts, faces, a.max_edge, attributes=attrs)
            print(f"max-edge: {s.rounds} rounds, longest edge {s.longest_edge}" + ("" if s.converged else " (not converged)"))
            verts, faces, attrs = s.verts, s.faces, s.attributes
        if a.subdivide is not None:
            s = meshclean.subdivide_mesh(verts, faces, a.subdivide, a.subdivide_scheme, attributes=attrs)
            verts, faces, attrs = s.verts, s.faces, s.attributes
        carried = None
        if attrs is not None:
            carried = attrs.cpu().numpy()
            if file_colors.dtype == np.uint8:                # a convex combination of 0..255 values is one
                carried = np.rint(np.clip(carried, 0.0, 255.0)).astype(np.uint8)
    if a.drop_self_intersections:
        n_before = verts.shape[0]
        verts, faces, n = meshclean.drop_self_intersections(verts, faces)
        print(f"drop_self_intersections: {n} faces dropped")
        if carried is not None and verts.shape[0] != n_before:
            print("drop_self_intersections: vertices were dropped, the file's colours are not carried")
            carried = None
    if a.orient or a.outward_from is not None:
        info = {}
        faces = meshclean.orient_faces(verts, faces, a.outward_from, _info=info).faces
        print(f"orient: {info['components']} components, {info['non_orientable']} not orientable, "
              f"{info['flipped']} faces flipped")
    normals = meshclean.vertex_normals(verts, faces).cpu().numpy() if a.normals else None
    colors = carried
    textured = None
    if a.colour or a.render or a.texture:
        unit = meshclean.vertex_normals(verts, faces, torch.float64)
        if a.colour or a.texture:
            images = torch.from_numpy(load_dtu_images(a.dtu_dir, a.scan)).to(dev)
            if images.shape[0] != mats.shape[0]:
                ap.error(f"{images.shape[0]} images for {mats.shape[0]} cameras")
        if a.texture:
            size = a.texture_size if a.texture_size is not None or a.texture_density is not None else 4096
            uv, texture, atlas, tex = _bake(verts, faces, mats, images, a.texture_density, size)
            write_obj(a.texture, verts.cpu().numpy(), faces.cpu().numpy(), uv, texture)
            owned = int((tex.n_seen >= 0).sum())
            print(f"texture: {atlas.W} x {atlas.H} texels at density {atlas.density:.6g}, {owned} owned, "
                  f"{int((tex.n_seen > 0).sum())} seen by a view -> {a.texture}")
            textured = (atlas, tex)
        if a.colour:
            colors, seen = meshrender.color_vertices(verts, faces, mats, images, normals=unit)
            print(f"colour: {int((seen > 0).sum())} of {verts.shape[0]} vertices seen by a view")
            colors = colors.cpu().numpy()
        if a.render:
            _write_renders(a.render, verts, faces, unit, mats, masks.shape[1], masks.shape[2], textured=textured)
    write_ply(a.output, verts.cpu().numpy(), faces.cpu().numpy(), normals, colors)
    print(f"{a.input}: {n0[0]} vertices, {n0[1]} faces -> {a.output}: {verts.shape[0]} vertices, {faces.shape[0]} faces")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
