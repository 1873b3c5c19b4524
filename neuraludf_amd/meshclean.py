"""Mesh clean-up on the GPU (csrc/meshtopo.hip): the steps between the mesher and the Chamfer evaluation that the
reference takes from trimesh, networkx, scipy.sparse and cv2.

    edge table   mesh_edges          unique undirected edges with their faces; boundary edges are those of count 1
    holes        fill_holes          extract_mesh.py:222-223 (trimesh fill_holes): loops of 3 get one triangle, of 4 two
    loops        border_loops, close_holes    the border as canonical closed loops and open chains, linked through the fans of
                                     the surface, and the loops of up to 64 edges closed with their minimum-area
                                     triangulation (csrc/meshhole.hip; MeshLab or pymeshfix on the CPU): the holes of 5 to
                                     30 edges that MeshUDF leaves where its gradient is unreliable
    crossings    close_holes_checked, drop_self_intersections    the patches that pass through the surface taken back, the
                                     faces that pass through or lie folded onto each other dropped
                                     (evaluation.self_intersections, csrc/meshintersect.hip; MeshLab or pymeshfix on the CPU)
    borders      smooth_borders      extract_mesh.py:238-265: 5 Jacobi steps of the border Laplacian, lambda = 0.3
    components   face_components, filter_components     clean_dtu_mesh.py:158-191
    orientation  orient_faces        consistent winding per component (csrc/meshorient.hip); the reference leaves it out
                                     (extract_mesh.py:218-219: trimesh's serial traversal is "too slow")
    normals      vertex_normals      extract_mesh.py:272-275 (trimesh weighted_vertex_normals, angle-weighted)
    smoothing    smooth_mesh, denoise_mesh, vertex_adjacency     Taubin's lambda | mu smoothing (uniform or cotangent) and the
                                     bilateral normal filter with its vertex update (csrc/meshsmooth.hip); the reference
                                     smooths the border only, its users take the rest to trimesh or open3d on the CPU
    simplify     simplify_mesh, simplify_to_faces    vertex clustering with quadric placement (csrc/meshsimplify.hip);
                                     the reference's users take this step to trimesh or open3d on the CPU
    measure      simplify_to_error, transfer_attributes   simplification to a measured two-sided deviation, attributes
                                     carried to the closest point of another mesh (evaluation.closest_on_mesh,
                                     csrc/meshdist.hip; trimesh.proximity.closest_point on the CPU)
    subdivide    subdivide_mesh, subdivide_to_edge    Loop and midpoint subdivision, and midpoint splits of the edges above
                                     a length (csrc/meshsubdiv.hip; trimesh.remesh.subdivide / subdivide_loop /
                                     subdivide_to_size on the CPU)
    remesh       remesh_isotropic    split, collapse, flip, relax and project towards well-shaped triangles of a requested
                                     edge length (csrc/meshremesh.hip; pymeshlab, CGAL or trimesh.remesh on the CPU)
    views        clean_by_views, clean_dtu_mesh         clean_dtu_mesh.py:36-154 (mask and visual-hull cleaning)
    masks        ellipse_footprint, dilate_masks, load_dtu_views

Device tensors in, device tensors out; empty meshes pass through unchanged.  Sorts and scans between the launches are
torch's (stable sort, integer prefix sums): every result is identical from run to run.

Where the definitions differ from the libraries the reference calls:
  * trimesh takes the boundary loops from a networkx cycle basis, which is not canonical where borders touch.  Here a hole
    is a closed loop of 3 or 4 boundary edges all of whose vertices have boundary degree exactly 2 (the loop is then a
    whole connected component of the boundary graph), and for a 3-loop the triangle must not exist already.  fill_holes
    leaves longer loops open.  The winding of a new face is a vote over its boundary edges (see fill_holes).
  * border_loops and close_holes do not go by the border degree: two border edges belong together at a vertex when the
    fan of faces around it leads from one to the other over edges with exactly two faces.  That is canonical where
    borders touch, does not look at the winding, and ends in an open chain where an edge with three faces or a face with a
    repeated vertex is in the way.  close_holes closes the closed loops of up to MAX_HOLE_EDGES = 64 edges (Barequet and
    Sharir's minimum-area triangulation, the area term of Liepa's weight) and says per loop why it did not; refining and
    fairing a patch is left to subdivide_to_edge and smooth_mesh(fixed=...).
  * two faces are adjacent when they share an undirected edge of any multiplicity; trimesh's face_adjacency pairs only
    the edges with exactly two faces.
  * orient_faces links faces over the edges with exactly two faces only (trimesh's face_adjacency, here on purpose: an
    edge with three faces says nothing about winding), never guesses on a component that cannot be oriented, and picks
    between the two consistent windings by a stated rule (trimesh keeps whatever its traversal meets first).
  * the structuring element is restated from the formula in OpenCV's documentation (ellipse_footprint); cv2 is not
    available to check it against.
"""
from __future__ import annotations

import glob
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr

MAX_VERTS = 1 << 31          # half-edge keys are min * V + max in int64
HULL_BORDER = 50             # clean_dtu_mesh.py:88
HULL_MAX_OUTSIDE = 5         # clean_dtu_mesh.py:105
SIMPLIFY_MAX_GRID = 1 << 20  # cells per axis: a cluster key (cx Gy + cy) Gz + cz stays below 2^60
SIMPLIFY_BISECT_ROUNDS = 24
MAX_HOLE_EDGES = _lib.HOLE_MAX_EDGES     # close_holes: W of the longest loop, 64 x 64 doubles, fits the LDS of a workgroup
# close_holes: the status of a border loop, the first that applies in the order of its docstring
HOLE_FILLED, HOLE_OPEN_CHAIN, HOLE_TOO_MANY_EDGES, HOLE_PERIMETER, HOLE_NONFINITE, HOLE_DUPLICATE, HOLE_REPEATED_VERTEX = (
    _lib.HOLE[k] for k in ("FILLED", "OPEN_CHAIN", "TOO_MANY_EDGES", "PERIMETER", "NONFINITE", "DUPLICATE", "REPEATED_VERTEX"))
HOLE_STATUS_NAMES = {v: k.lower() for k, v in _lib.HOLE.items()}


class EdgeTable(NamedTuple):
    """edges [E, 5] int64: (u, v, count, first face, second face or -1) per unique undirected edge, u <= v, ordered by
    (u, v); he_edge [3 F]: row of the edge of half-edge 3 f + k (faces[f][k] -> faces[f][(k + 1) % 3]); he_key / he_id
    [3 F]: the sorted keys u * V + v and the half-edge at each sorted position; edge_start / edge_key [E]: first sorted
    position and key of each edge"""
    edges: torch.Tensor
    he_edge: torch.Tensor
    he_key: torch.Tensor
    he_id: torch.Tensor
    edge_start: torch.Tensor
    edge_key: torch.Tensor


def _check_faces(faces, n_verts):
    if not isinstance(faces, torch.Tensor):
        raise ValueError("faces must be a torch tensor")
    if faces.dtype != torch.int64:
        raise ValueError(f"faces must be int64 (got {faces.dtype})")
    if not faces.is_cuda:
        raise ValueError(f"faces must be on a GPU (got {faces.device})")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be [F, 3] (got {tuple(faces.shape)})")
    n_verts = int(n_verts)
    if not 0 <= n_verts < MAX_VERTS:
        raise ValueError(f"n_verts {n_verts} outside [0, 2^31)")
    if faces.shape[0]:
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= n_verts:
            raise ValueError(f"face index out of range: [{lo}, {hi}] for {n_verts} vertices")
    return faces.contiguous(), n_verts


def _check_mesh(verts, faces):
    if not isinstance(verts, torch.Tensor):
        raise ValueError("verts must be a torch tensor")
    if verts.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"verts must be float32 or float64 (got {verts.dtype})")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    faces, _ = _check_faces(faces, verts.shape[0])
    if verts.device != faces.device:
        raise ValueError(f"verts and faces must be on the same GPU (got {verts.device}, {faces.device})")
    return verts.contiguous(), faces


def _topo(faces, n_verts, table=None):
    d = _lib.MeshTopo(faces=ptr(faces), n_faces=faces.shape[0], n_verts=n_verts)
    if table is not None:
        d.he_key, d.he_id, d.edge_start = ptr(table.he_key), ptr(table.he_id), ptr(table.edge_start)
        d.edges, d.he_edge, d.edge_key = ptr(table.edges), ptr(table.he_edge), ptr(table.edge_key)
        d.n_edges = table.edges.shape[0]
    return d


def mesh_edges(faces, n_verts):
    """edge table of a triangle mesh -> EdgeTable.  faces: [F, 3] int64 on a GPU over n_verts < 2^31 vertices."""
    faces, n_verts = _check_faces(faces, n_verts)
    return _mesh_edges(faces, n_verts)


def _mesh_edges(faces, n_verts):
    dev = faces.device
    a, b = faces.reshape(-1), faces.roll(-1, 1).reshape(-1)
    he_key, he_id = torch.sort(torch.minimum(a, b) * n_verts + torch.maximum(a, b), stable=True)
    first = torch.ones(he_key.numel(), dtype=torch.bool, device=dev)
    if he_key.numel():
        first[1:] = he_key[1:] != he_key[:-1]
    edge_start = torch.nonzero(first).reshape(-1)
    table = EdgeTable(torch.empty((edge_start.numel(), 5), dtype=torch.int64, device=dev),
                      torch.empty(he_key.numel(), dtype=torch.int64, device=dev), he_key, he_id, edge_start,
                      he_key[edge_start])
    call("nudf_meshtopo_edges", _topo(faces, n_verts, table))
    return table


class _Boundary(NamedTuple):
    nbr_off: torch.Tensor      # [V + 1] CSR offsets
    nbr: torch.Tensor          # boundary neighbours of each vertex, ascending
    bverts: torch.Tensor       # vertices with a boundary edge, ascending
    n_edges: int


def _boundary(table, n_verts):
    """CSR of the boundary graph (edges of count 1): a sort of the 2 B directed pairs, a count and a scan"""
    e = table.edges
    b = e[e[:, 2] == 1]
    key = torch.sort(torch.cat([b[:, 0] * n_verts + b[:, 1], b[:, 1] * n_verts + b[:, 0]])).values
    src = key // n_verts if n_verts else key
    deg = torch.bincount(src, minlength=n_verts)
    nbr_off = torch.zeros(n_verts + 1, dtype=torch.int64, device=e.device)
    torch.cumsum(deg, 0, out=nbr_off[1:])
    nbr = (key - src * n_verts).contiguous()
    return _Boundary(nbr_off, nbr, torch.nonzero(deg).reshape(-1), b.shape[0])


def boundary_degree(faces, n_verts):
    """-> [V] int64: number of boundary edges (edges with exactly one face) at each vertex"""
    faces, n_verts = _check_faces(faces, n_verts)
    off = _boundary(_mesh_edges(faces, n_verts), n_verts).nbr_off
    return off[1:] - off[:-1]


def fill_holes(verts, faces, max_loop=4):
    """closes the holes of 3 (one triangle) and, with max_loop = 4, of 4 boundary edges (two triangles, split along the
    shorter diagonal in float64; tie: the diagonal through the smallest vertex index) -> (faces' [F + n, 3], number of
    holes filled).  A hole is a closed loop of boundary edges whose vertices all have boundary degree 2; a 3-loop whose
    triangle is already a face is left.  A new face starts at its smallest vertex and ascends, unless more of its boundary
    edges run in that direction in the face next to them than against it (trimesh's rule as a vote: MeshUDF meshes are
    not consistently wound).  New faces follow the old ones, ordered by their smallest vertex.  One pass: a filled hole
    makes no new boundary."""
    if max_loop not in (3, 4):
        raise ValueError(f"max_loop must be 3 or 4 (got {max_loop})")
    verts, faces = _check_mesh(verts, faces)
    if faces.shape[0] == 0:
        return faces, 0
    n_verts = verts.shape[0]
    table = _mesh_edges(faces, n_verts)
    bd = _boundary(table, n_verts)
    if bd.bverts.numel() == 0:
        return faces, 0
    pos = verts.double().contiguous()
    count = torch.empty(bd.bverts.numel(), dtype=torch.int64, device=faces.device)
    d = _topo(faces, n_verts, table)
    d.nbr_off, d.nbr, d.bverts, d.n_bverts = ptr(bd.nbr_off), ptr(bd.nbr), ptr(bd.bverts), bd.bverts.numel()
    d.pos, d.max_loop, d.new_count = ptr(pos), max_loop, ptr(count)
    call("nudf_meshtopo_fill_count", d)
    ends = torch.cumsum(count, 0)
    n_new = int(ends[-1])
    if n_new == 0:
        return faces, 0
    off = ends - count
    new = torch.empty((n_new, 3), dtype=torch.int64, device=faces.device)
    d.new_off, d.new_faces, d.n_new = ptr(off), ptr(new), n_new
    call("nudf_meshtopo_fill_emit", d)
    return torch.cat([faces, new]), int((count > 0).sum())


class BorderLoops(NamedTuple):
    """loop_off [L + 1] CSR offsets; loop_vertex: the vertex at which each border edge is entered, in the loop's canonical
    order (edge i runs from loop_vertex[i] to loop_vertex[i + 1], the last of a closed loop back to the first; the far end of
    a chain's last edge is not listed); loop_edge: the rows of the EdgeTable, same CSR; closed [L] bool; perimeter [L]
    float64, the edge lengths summed in loop order; edge_loop [E] int64: the loop of each border edge, -1 for other edges"""
    loop_off: torch.Tensor
    loop_vertex: torch.Tensor
    loop_edge: torch.Tensor
    closed: torch.Tensor
    perimeter: torch.Tensor
    edge_loop: torch.Tensor


class ClosedHoles(NamedTuple):
    """faces [F + n, 3] int64, the input's followed by the patches loop by loop in loop-id order; new_face_loop [n] int64:
    the loop (border_loops' id) each new face closes; status [L] int8: one HOLE_ code per loop"""
    faces: torch.Tensor
    new_face_loop: torch.Tensor
    status: torch.Tensor


def _hole_loops(d, table, n_verts, events=None, state=None, _rounds=None):
    """link, the rank rounds and the glue between and after them -> (loop_off, loop_vertex, loop_edge, closed uint8,
    edge_loop, link); d holds the mesh and its table and receives the border lists, which the caller keeps alive through the
    returned tuple's last entry"""
    e, dev = table.edges, table.edges.device
    n_edges = e.shape[0]
    _stage(events, state, "glue")
    bedge = torch.nonzero(e[:, 2] == 1).reshape(-1)
    n_border = bedge.numel()
    brank = torch.full((n_edges,), -1, dtype=torch.int64, device=dev)
    brank[bedge] = torch.arange(n_border, dtype=torch.int64, device=dev)
    link = torch.empty(2 * n_border, dtype=torch.int64, device=dev)
    d.sp_sd_hf_bedge, d.sp_sd_hf_brank, d.sp_sd_hf_link, d.sp_sd_hf_n_border = ptr(bedge), ptr(brank), ptr(link), n_border
    _stage(events, state, "link")
    call("nudf_meshhole_link", d)
    _stage(events, state, "glue2")
    s = torch.arange(2 * n_border, dtype=torch.int64, device=dev)
    over = link[s ^ 1]
    tab = torch.stack([torch.where(over >= 0, over, s ^ 1), s, torch.zeros_like(s)], 1).contiguous()
    other = torch.empty_like(tab)
    _stage(events, state, "rank")
    for r in range((2 * n_border - 1).bit_length() + 1 if n_border else 0):
        d.sp_sd_hf_rank_in, d.sp_sd_hf_rank_out, d.sp_sd_hf_round = ptr(tab), ptr(other), r
        call("nudf_meshhole_rank", d)
        tab, other = other, tab
        if _rounds is not None:
            _rounds.append(tab.clone())
    _stage(events, state, "glue3")
    # every state lies on a cycle (a closed loop: one per direction; a chain: there and back): m its smallest state, dist
    # the steps to it
    m, dist = tab[:, 1], tab[:, 2]
    n = 2 * n_border
    chain = m == m[s ^ 1]
    length = torch.bincount(m, minlength=n)[m]
    first = torch.full((n,), n, dtype=torch.int64, device=dev)           # per cycle: the smaller of a chain's two start states
    starts = s[link < 0]
    by_cycle = torch.sort(m[starts], stable=True)                         # starts ascend: the first of a cycle is the smaller
    lead = torch.ones(starts.numel(), dtype=torch.bool, device=dev)
    if starts.numel():
        lead[1:] = by_cycle.values[1:] != by_cycle.values[:-1]
    first[by_cycle.values[lead]] = starts[by_cycle.indices[lead]]
    origin = torch.where(chain, first[m], m)
    origin = torch.where(origin < n, origin, m)
    pos = torch.remainder(dist[origin] - dist, length)
    canonical = torch.where(chain, 2 * pos < length, m < m[s ^ 1])
    label = torch.minimum(m, m[s ^ 1]) >> 1                                # the loop's smallest border edge
    cs = s[canonical]
    cs = cs[torch.sort(pos[cs], stable=True).indices]
    cs = cs[torch.sort(label[cs], stable=True).indices]
    lab = label[cs]
    head = torch.ones(cs.numel(), dtype=torch.bool, device=dev)
    if cs.numel():
        head[1:] = lab[1:] != lab[:-1]
    start = torch.nonzero(head).reshape(-1)
    loop_off = torch.cat([start, torch.full((1,), cs.numel(), dtype=torch.int64, device=dev)])
    loop_edge = bedge[cs >> 1].contiguous()
    loop_vertex = e[loop_edge, cs & 1].contiguous()
    closed = (~chain[cs[start]]).to(torch.uint8).contiguous()
    edge_loop = torch.full((n_edges,), -1, dtype=torch.int64, device=dev)
    edge_loop[loop_edge] = torch.cumsum(head, 0) - 1
    return loop_off, loop_vertex, loop_edge, closed, edge_loop, (bedge, brank, link)


def _hole_count(d, pos, loops, max_edges, max_perimeter):
    """launches count -> (perimeter [L], status [L] int8, new_count [L]); d keeps pointers into `loops`"""
    loop_off, loop_vertex, loop_edge, closed = loops[:4]
    n_loops, dev = closed.numel(), closed.device
    perimeter = torch.empty(n_loops, dtype=torch.float64, device=dev)
    status = torch.empty(n_loops, dtype=torch.int8, device=dev)
    count = torch.empty(n_loops, dtype=torch.int64, device=dev)
    d.pos, d.max_loop, d.sp_sd_hf_max_perimeter = ptr(pos), max_edges, math.inf if max_perimeter is None else max_perimeter
    d.sp_sd_hf_loop_off, d.sp_sd_hf_loop_vertex, d.sp_sd_hf_loop_edge = ptr(loop_off), ptr(loop_vertex), ptr(loop_edge)
    d.sp_sd_hf_closed, d.sp_sd_hf_n_loops, d.sp_sd_hf_n_items = ptr(closed), n_loops, loop_edge.numel()
    d.sp_sd_hf_perimeter, d.sp_sd_hf_status, d.new_count = ptr(perimeter), ptr(status), ptr(count)
    call("nudf_meshhole_count", d)
    return perimeter, status, count


def _empty_loops(n_edges, dev):
    z = torch.zeros(0, dtype=torch.int64, device=dev)
    return BorderLoops(torch.zeros(1, dtype=torch.int64, device=dev), z, z.clone(), torch.zeros(0, dtype=torch.bool, device=dev),
                       torch.zeros(0, dtype=torch.float64, device=dev), torch.full((n_edges,), -1, dtype=torch.int64, device=dev))


def border_loops(verts, faces):
    """the border of the mesh as closed loops and open chains -> BorderLoops (csrc/meshhole.hip).  A border edge is an edge
    with one face.  At each of its two ends the fan of the surface is walked: from the edge's face across the face's other
    edge at that vertex into the next face, for as long as that edge has exactly two faces.  The first edge with one face
    is the border edge linked to this one at this end; an edge with three or more faces blocks the end, as does a face
    with a repeated vertex.  The link is mutual and does not look at the winding, so the border edges fall into disjoint
    closed loops and into open chains whose two ends are blocked; borders that touch in a vertex come apart into the loops
    that the surface around the vertex dictates (trimesh takes the loops from a cycle basis, which is not canonical there).
    Loops are numbered by their smallest border edge (row of the EdgeTable).  A closed loop starts with that edge, entered
    at its smaller vertex; a chain starts at the one of its two blocked ends whose (edge, end) pair is smaller.  Found by
    pointer doubling over the (edge, direction) states, ceil(log2(2 B)) + 1 rounds for B border edges, with stable sorts
    and scans in torch between the launches: identical from run to run, and unchanged by flipping faces."""
    verts, faces = _check_mesh(verts, faces)
    n_verts, dev = verts.shape[0], faces.device
    if faces.shape[0] == 0:
        return _empty_loops(0, dev)
    table = _mesh_edges(faces, n_verts)
    d = _topo(faces, n_verts, table)
    loops = _hole_loops(d, table, n_verts)
    if loops[3].numel() == 0:
        return _empty_loops(table.edges.shape[0], dev)
    perimeter, _, _ = _hole_count(d, verts.double().contiguous(), loops, MAX_HOLE_EDGES, None)
    return BorderLoops(loops[0], loops[1], loops[2], loops[3].bool(), perimeter, loops[4])


def _shared_patch_edges(new, face_loop, n_verts):
    """the loops whose patch has an edge that the patch of a loop with a smaller id has too (two holes through the same two
    vertices): one stable sort of the patches' half-edge keys"""
    a, b = new.reshape(-1), new.roll(-1, 1).reshape(-1)
    key, loop = torch.minimum(a, b) * n_verts + torch.maximum(a, b), face_loop.repeat_interleave(3)
    sk, order = torch.sort(key, stable=True)
    sl = loop[order]                                   # ascending inside a key: the rows are in loop order
    first = torch.ones(sk.numel(), dtype=torch.bool, device=new.device)
    first[1:] = sk[1:] != sk[:-1]
    owner = sl[first][torch.cumsum(first, 0) - 1]
    return torch.unique(sl[sl != owner])


def close_holes(verts, faces, max_edges=32, max_perimeter=None, _info=None):
    """closes the border loops (border_loops) of up to `max_edges` <= MAX_HOLE_EDGES = 64 edges with their minimum-area
    triangulation -> ClosedHoles(faces, new_face_loop, status) (csrc/meshhole.hip; MeshLab's and pymeshfix's hole filling on
    the CPU; fill_holes, which mirrors trimesh, stops at 4 edges and at borders that touch).  status [L] holds one code per
    loop, the first that applies: HOLE_OPEN_CHAIN (not a closed loop), HOLE_TOO_MANY_EDGES, HOLE_REPEATED_VERTEX (the loop
    passes a vertex twice: left open), HOLE_NONFINITE (a coordinate or the perimeter), HOLE_PERIMETER (perimeter above
    `max_perimeter`, when given), HOLE_DUPLICATE (the patch would duplicate an edge or face, see below), else HOLE_FILLED.
    A loop v_0 ... v_n-1 in canonical order gets the triangulation of least total area (Barequet and Sharir; the area
    term of Liepa's weight, without the dihedral term): W[i][i + 1] = 0, W[i][j] = min over i < k < j of
    (W[i][k] + W[k][j]) + A(i, k, j) with A = 0.5 sqrt(|(v_k - v_i) x (v_j - v_i)|^2) in float64, k ascending, the first
    strictly smaller value wins; the n - 2 triangles follow in pre-order from (0, n - 1): (i, k, j), then those of (i, k),
    then those of (k, j).  Winding: a triangle is (v_i, v_k, v_j) unless more than half of the loop's border edges run in
    loop direction in the face next to them, then (v_i, v_j, v_k): the patch runs against the majority of its neighbours
    (the vote of fill_holes), a tie keeps the loop's direction.  Refusal: when a diagonal of the chosen triangulation is an
    edge of the mesh already, or a 3-loop is the border of a single face, the loop is left open whole; so is a loop whose
    patch shares an edge with the patch of a loop of smaller id.  No edge gains a third face.  One pass: a patch makes no
    new border.  The patches are as coarse as their loops: refine and fair them with subdivide_to_edge and
    smooth_mesh(fixed=...) with every old vertex fixed.  Identical from run to run; unchanged in its set of filled loops by
    relabelling the vertices.  (`_info`: a dict that receives loops (BorderLoops) and, when it holds a dict under
    "events", a pair of events per stage.)"""
    try:
        ok = int(max_edges) == max_edges and 3 <= int(max_edges) <= MAX_HOLE_EDGES
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"max_edges must be an integer in [3, {MAX_HOLE_EDGES}] (got {max_edges!r})")
    max_edges = int(max_edges)
    if max_perimeter is not None:
        max_perimeter = _finite(max_perimeter, "max_perimeter", positive=True)
    verts, faces = _check_mesh(verts, faces)
    n_verts, dev = verts.shape[0], faces.device
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    events, state = None if _info is None else _info.get("events"), {}
    if faces.shape[0] == 0:
        if _info is not None:
            _info["loops"] = _empty_loops(0, dev)
        return ClosedHoles(faces, none, torch.zeros(0, dtype=torch.int8, device=dev))
    _stage(events, state, "edges")
    table = _mesh_edges(faces, n_verts)
    d = _topo(faces, n_verts, table)
    loops = _hole_loops(d, table, n_verts, events, state)
    if loops[3].numel() == 0:
        _stage(events, state, None)
        if _info is not None:
            _info["loops"] = _empty_loops(table.edges.shape[0], dev)
        return ClosedHoles(faces, none, torch.zeros(0, dtype=torch.int8, device=dev))
    pos = verts.double().contiguous()
    _stage(events, state, "count")
    perimeter, status, count = _hole_count(d, pos, loops, max_edges, max_perimeter)
    if _info is not None:
        _info["loops"] = BorderLoops(loops[0], loops[1], loops[2], loops[3].bool(), perimeter, loops[4])
    _stage(events, state, "glue4")
    ends = torch.cumsum(count, 0)
    n_new = int(ends[-1])
    if n_new == 0:
        _stage(events, state, None)
        return ClosedHoles(faces, none, status)
    off = ends - count
    new = torch.full((n_new, 3), -1, dtype=torch.int64, device=dev)
    d.new_off, d.new_faces, d.n_new = ptr(off), ptr(new), n_new
    _stage(events, state, "triangulate")
    call("nudf_meshhole_triangulate", d)
    _stage(events, state, "glue5")
    face_loop = torch.arange(count.numel(), dtype=torch.int64, device=dev).repeat_interleave(count)
    keep = new[:, 0] >= 0
    new, face_loop = new[keep], face_loop[keep]
    bad = _shared_patch_edges(new, face_loop, n_verts)
    if bad.numel():
        status[bad] = HOLE_DUPLICATE
        keep = ~torch.isin(face_loop, bad)
        new, face_loop = new[keep], face_loop[keep]
    out = ClosedHoles(torch.cat([faces, new]), face_loop, status)
    _stage(events, state, None)
    return out


def _isect_kinds(kinds):
    from . import evaluation                                 # lazily: evaluation imports meshing, which imports this file
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    for k in kinds:
        if k not in evaluation.ISECT_KINDS:
            raise ValueError(f"kinds must be among {tuple(evaluation.ISECT_KINDS)} (got {k!r})")
    return [evaluation.ISECT_KINDS[k] for k in kinds]


def _pairs_of_kinds(res, kinds):
    """the pairs of an evaluation.Intersections whose kind is one of the codes `kinds`"""
    hit = torch.zeros_like(res.kind, dtype=torch.bool)
    for k in kinds:
        hit |= res.kind == k
    return res.pairs[hit]


def drop_self_intersections(verts, faces, kinds=("crossing", "coplanar")):
    """drops every face that is in a pair of evaluation.self_intersections of one of `kinds` ("crossing", "coplanar",
    "uncertain"; csrc/meshintersect.hip), then the vertices no face uses any more (compact_mesh) -> (verts', faces', the
    number of faces dropped).  Both faces of a pair go: which of the two is the wrong one is not a question signs answer.
    Dropping faces makes no new pair, so a second call finds nothing of these kinds.  The repair stops here: the holes
    this leaves are border loops like any other (close_holes)."""
    from . import evaluation
    codes = _isect_kinds(kinds)
    verts, faces = _check_mesh(verts, faces)
    if faces.shape[0] == 0:
        return verts, faces, 0
    res = evaluation.self_intersections(verts, faces)
    keep = torch.ones(faces.shape[0], dtype=torch.bool, device=faces.device)
    keep[_pairs_of_kinds(res, codes).reshape(-1)] = False
    dropped = int((~keep).sum())
    if dropped == 0:
        return verts, faces, 0
    return compact_mesh(verts, faces, face_mask=keep) + (dropped,)


def close_holes_checked(verts, faces, max_edges=32, max_perimeter=None):
    """close_holes, then evaluation.self_intersections on the closed mesh: the patch of every loop that has a new face in a
    "crossing" or "coplanar" pair -- with an old face or with a face of another patch -- is taken back whole, since the
    minimum-area triangulation of a rim looks at the rim alone and can cut through the surface next to it or through
    something standing in the hole -> (ClosedHoles of what is kept, the ids [K] int64 of the loops taken back,
    ascending).  The status of a loop taken back stays what close_holes gave it (HOLE_FILLED); its faces are gone from
    `faces` and `new_face_loop`.  Pairs among the old faces take nothing back: they were there before."""
    from . import evaluation
    closed = close_holes(verts, faces, max_edges, max_perimeter)
    n_old, n_new = faces.shape[0], closed.new_face_loop.numel()
    none = torch.zeros(0, dtype=torch.int64, device=closed.faces.device)
    if n_new == 0:
        return closed, none
    res = evaluation.self_intersections(verts, closed.faces)
    hit = _pairs_of_kinds(res, _isect_kinds(("crossing", "coplanar"))).reshape(-1)
    hit = hit[hit >= n_old] - n_old
    if hit.numel() == 0:
        return closed, none
    bad = torch.unique(closed.new_face_loop[hit])
    keep = ~torch.isin(closed.new_face_loop, bad)
    kept = torch.cat([closed.faces[:n_old], closed.faces[n_old:][keep]])
    return ClosedHoles(kept, closed.new_face_loop[keep], closed.status), bad


def smooth_borders(verts, faces, iterations=5, lam=0.3):
    """Laplacian smoothing of the border vertices along the border -> verts' [V, 3] float32.  Each of `iterations` Jacobi
    steps moves every vertex with a boundary edge by lam times the difference between the mean of its neighbours along
    boundary edges and itself, all from the previous step's positions; float64 inside, neighbours summed in ascending
    index, cast to float32 at the end only.  Other vertices do not move."""
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"iterations must be >= 0 (got {iterations})")
    verts, faces = _check_mesh(verts, faces)
    if faces.shape[0] == 0 or iterations == 0:
        return verts.float()
    n_verts = verts.shape[0]
    bd = _boundary(_mesh_edges(faces, n_verts), n_verts)
    if bd.bverts.numel() == 0:
        return verts.float()
    pos = verts.double().contiguous()                # may be the caller's tensor: read only
    bufs = [pos.clone(), pos.clone() if iterations > 1 else None]      # a step writes the border rows only
    d = _topo(faces, n_verts)
    d.nbr_off, d.nbr, d.bverts, d.n_bverts, d.lam = ptr(bd.nbr_off), ptr(bd.nbr), ptr(bd.bverts), bd.bverts.numel(), lam
    for i in range(iterations):
        d.pos, d.pos_out = ptr(pos), ptr(bufs[i % 2])
        call("nudf_meshtopo_smooth", d)
        pos = bufs[i % 2]
    return pos.float()


def face_components(faces, n_verts, _info=None):
    """connected components over faces -> labels [F] int64: the smallest face index of each face's component.  Two faces
    are adjacent when they share an undirected edge, whatever the number of faces on it (trimesh's face_adjacency, which
    the reference uses, pairs only the edges with exactly two faces).  Rounds of min-label hooking over the sorted
    half-edges and pointer jumping, one 4-byte read-back per round.  (`_info`: a dict that receives the number of rounds.)"""
    faces, n_verts = _check_faces(faces, n_verts)
    return _face_components(faces, n_verts, _mesh_edges(faces, n_verts) if faces.shape[0] else None, _info)


def _face_components(faces, n_verts, table, _info=None):
    n = faces.shape[0]
    labels = torch.arange(n, dtype=torch.int64, device=faces.device)
    rounds = 0
    if n:
        changed = torch.zeros(1, dtype=torch.int32, device=faces.device)
        d = _topo(faces, n_verts, table)
        d.labels, d.changed = ptr(labels), ptr(changed)
        while True:
            if rounds > n:                                   # every round that changes something lowers a label
                raise RuntimeError("face_components did not converge")
            changed.zero_()
            call("nudf_meshtopo_cc_hook", d)
            call("nudf_meshtopo_cc_jump", d)
            rounds += 1
            if int(changed.item()) == 0:
                break
    if _info is not None:
        _info["rounds"] = rounds
    return labels


class Orientation(NamedTuple):
    """faces [F, 3] int64 with the chosen faces flipped ([a, b, c] -> [a, c, b]); flipped [F] bool; labels [F] int64: the
    smallest face index of each face's orientation component; orientable [F] bool: the verdict on the face's component"""
    faces: torch.Tensor
    flipped: torch.Tensor
    labels: torch.Tensor
    orientable: torch.Tensor


def _check_origin(outward_from):
    if outward_from is None:
        return None
    try:
        o = [float(x) for x in outward_from]
    except (TypeError, ValueError):
        raise ValueError(f"outward_from must be three finite numbers (got {outward_from!r})") from None
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError(f"outward_from must be three finite numbers (got {outward_from!r})")
    return o


def _manifold_edges(faces, n_verts):
    """the two half-edges of every manifold edge -> (me_a [M], me_b [M]), ordered by edge key: an undirected edge with
    exactly two half-edges, of two different faces neither of which repeats a vertex"""
    a, b = faces.reshape(-1), faces.roll(-1, 1).reshape(-1)
    he_key, he_id = torch.sort(torch.minimum(a, b) * n_verts + torch.maximum(a, b), stable=True)
    eq = he_key[1:] == he_key[:-1]
    pair = eq.clone()                                 # position j: keys j and j + 1 are equal and no neighbour joins them
    pair[1:] &= ~eq[:-1]
    pair[:-1] &= ~eq[1:]
    j = torch.nonzero(pair).reshape(-1)
    ha, hb = he_id[j], he_id[j + 1]
    degenerate = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    fa, fb = ha // 3, hb // 3
    keep = (fa != fb) & ~degenerate[fa] & ~degenerate[fb]
    return ha[keep].contiguous(), hb[keep].contiguous()


def orient_faces(verts, faces, outward_from=None, _info=None):
    """winds the faces of every orientable component consistently -> Orientation(faces, flipped, labels, orientable).
    Two faces across a manifold edge (exactly two half-edges, of two different faces without a repeated vertex) are
    compatible when they run along it in opposite directions; a component is a set of faces connected over manifold edges
    (border edges and edges with three or more faces connect nothing; a face with a repeated vertex is a component of its
    own and is never flipped), labelled by its smallest face index.  An orientable component has exactly two sets of flips
    that make all its manifold edges compatible, each the complement of the other: the one that flips fewer faces is
    taken, on a tie the one that leaves the component's smallest face alone.  With outward_from = (x, y, z) the set for
    which S = sum_f N_f . (c_f - outward_from) is positive is taken instead (N_f = (p1 - p0) x (p2 - p0) after the flips,
    c_f = (p0 + (p1 + p2)) / 3, float64, summed in a fixed order: the other set gives exactly -S); where S is 0 or not
    finite the first rule decides.  A component that cannot be oriented is returned as it came and reported in
    `orientable`.  A flip is [a, b, c] -> [a, c, b]: faces keep their order and their first vertex.  A parity union-find
    over the faces: rounds of hooking over the manifold edges and pointer jumping as in face_components, one 4-byte
    read-back per round; the result does not depend on the order in which the atomics land.  (`_info`: a dict that
    receives rounds, components, orientable, non_orientable, flipped.)"""
    verts, faces = _check_mesh(verts, faces)
    origin = _check_origin(outward_from)
    n, n_verts, dev = faces.shape[0], verts.shape[0], faces.device
    info = dict(rounds=0, components=0, orientable=0, non_orientable=0, flipped=0)
    if n == 0:
        if _info is not None:
            _info.update(info)
        none = torch.zeros(0, dtype=torch.bool, device=dev)
        return Orientation(faces, none, torch.zeros(0, dtype=torch.int64, device=dev), none.clone())
    me_a, me_b = _manifold_edges(faces, n_verts)
    word = torch.arange(n, dtype=torch.int64, device=dev) * 2
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    nonorient = torch.zeros(n, dtype=torch.uint8, device=dev)
    d = _lib.MeshOrient(faces=ptr(faces), me_a=ptr(me_a), me_b=ptr(me_b), word=ptr(word), changed=ptr(changed),
                        nonorient=ptr(nonorient), n_faces=n, n_verts=n_verts, n_medges=me_a.numel())
    rounds = 0
    while me_a.numel():
        if rounds > n:                                       # every round that changes something lowers a parent
            raise RuntimeError("orient_faces did not converge")
        changed.zero_()
        call("nudf_meshorient_hook", d)
        call("nudf_meshorient_jump", d)
        rounds += 1
        if int(changed.item()) == 0:
            break
    call("nudf_meshorient_check", d)
    labels, parity = word >> 1, (word & 1).bool()
    orientable = nonorient[labels] == 0
    size = torch.bincount(labels, minlength=n)
    complement = 2 * torch.bincount(labels[parity], minlength=n) > size       # per label: the other set flips fewer faces
    if origin is not None:
        comps = torch.nonzero(size).reshape(-1)
        comp_off = torch.zeros(comps.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(size[comps], 0, out=comp_off[1:])
        comp_face = torch.sort(labels, stable=True).indices              # ascending face index inside a component
        pos = verts.double().contiguous()
        comp_sum = torch.empty(comps.numel(), dtype=torch.float64, device=dev)
        d.comp_off, d.comp_face, d.comp_sum, d.pos, d.n_comps = ptr(comp_off), ptr(comp_face), ptr(comp_sum), ptr(pos), \
            comps.numel()
        d.origin[0], d.origin[1], d.origin[2] = origin
        call("nudf_meshorient_outward", d)
        decides = torch.isfinite(comp_sum) & (comp_sum != 0)
        complement[comps] = torch.where(decides, comp_sum < 0, complement[comps])
    flipped = (parity ^ complement[labels]) & orientable
    out = torch.where(flipped[:, None], faces[:, [0, 2, 1]], faces)
    if _info is not None:
        info.update(rounds=rounds, components=int((size > 0).sum()), non_orientable=int(nonorient.sum()),
                    flipped=int(flipped.sum()))
        info["orientable"] = info["components"] - info["non_orientable"]
        _info.update(info)
    return Orientation(out, flipped, labels, orientable)


def _corner_lists(faces, n_verts):
    """-> (corner_off [V + 1], corner [3 F]): the corners 3 f + k by vertex, ascending inside each"""
    flat = faces.reshape(-1)
    corner = torch.sort(flat, stable=True).indices
    corner_off = torch.zeros(n_verts + 1, dtype=torch.int64, device=faces.device)
    torch.cumsum(torch.bincount(flat, minlength=n_verts), 0, out=corner_off[1:])
    return corner_off, corner


def vertex_normals(verts, faces, dtype=torch.float32):
    """angle-weighted vertex normals -> [V, 3] `dtype` (float32 or float64), computed in float64 and cast at the end:
    trimesh's weighted_vertex_normals, which the reference calls (extract_mesh.py:272-275).  With n_f = (p1 - p0) x
    (p2 - p0) of face f, a face whose |n_f| is 0 or not finite adds nothing; at corner k of f the weight is theta =
    atan2(|n_f|, e1 . e2), e1 / e2 the edges from the corner to the next / previous vertex of the face; N_v = the sum of
    theta * (n_f / |n_f|) over the corners at v in ascending 3 f + k, and the result N_v / |N_v|, or (0, 0, 0) where
    |N_v| is 0 or not finite or no face uses the vertex.  The normals follow the winding: orient_faces first."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64 (got {dtype})")
    verts, faces = _check_mesh(verts, faces)
    n_verts, dev = verts.shape[0], verts.device
    normals = torch.zeros((n_verts, 3), dtype=torch.float64, device=dev)
    if n_verts == 0 or faces.shape[0] == 0:
        return normals.to(dtype)
    pos = verts.double().contiguous()
    corner_off, corner = _corner_lists(faces, n_verts)
    d = _lib.MeshOrient(faces=ptr(faces), pos=ptr(pos), corner_off=ptr(corner_off), corner=ptr(corner),
                        normals=ptr(normals), n_faces=faces.shape[0], n_verts=n_verts)
    call("nudf_meshorient_normals", d)
    return normals.to(dtype)


def vertex_adjacency(faces, n_verts, table=None):
    """the one-ring of every vertex -> (nbr_off [V + 1], nbr) int64, a CSR with the neighbours of each vertex ascending:
    the other ends of the unique edges at the vertex (an edge from a vertex to itself, which a face with a repeated vertex
    has, is none).  Both directions of the edge table's rows under one stable key sort; `table`: the mesh's EdgeTable
    where the caller has one."""
    faces, n_verts = _check_faces(faces, n_verts)
    return _vertex_adjacency(faces, n_verts, table)


def _vertex_adjacency(faces, n_verts, table=None):
    dev = faces.device
    nbr_off = torch.zeros(n_verts + 1, dtype=torch.int64, device=dev)
    if faces.shape[0] == 0 or n_verts == 0:
        return nbr_off, torch.zeros(0, dtype=torch.int64, device=dev)
    e = (table if table is not None else _mesh_edges(faces, n_verts)).edges
    e = e[e[:, 0] != e[:, 1]]
    key = torch.sort(torch.cat([e[:, 0] * n_verts + e[:, 1], e[:, 1] * n_verts + e[:, 0]]), stable=True).values
    src = key // n_verts
    torch.cumsum(torch.bincount(src, minlength=n_verts), 0, out=nbr_off[1:])
    return nbr_off, (key - src * n_verts).contiguous()


def _count(x, name):
    try:
        n = int(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integer >= 0 (got {x!r})") from None
    if n < 0 or n != x:
        raise ValueError(f"{name} must be an integer >= 0 (got {x!r})")
    return n


def _finite(x, name, positive=False):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite number (got {x!r})") from None
    if not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"{name} must be a {'positive ' if positive else ''}finite number (got {x!r})")
    return v


def _fixed_mask(verts, table, boundary, fixed):
    """the vertices that keep their positions -> uint8 [V], or None when there are none to keep: the caller's mask and,
    with boundary="fixed", the ends of the edges with one face"""
    if boundary not in ("fixed", "free"):
        raise ValueError(f"boundary must be 'fixed' or 'free' (got {boundary!r})")
    n_verts, dev = verts.shape[0], verts.device
    mask = None
    if fixed is not None:
        mask = torch.as_tensor(fixed, device=dev)
        if mask.dim() != 1 or mask.shape[0] != n_verts or mask.is_floating_point() or mask.is_complex():
            raise ValueError(f"fixed must be a [{n_verts}] boolean mask (got {mask.dtype} {tuple(mask.shape)})")
        mask = mask != 0
    if boundary == "fixed" and table is not None:
        e = table.edges
        b = e[e[:, 2] == 1]
        mask = torch.zeros(n_verts, dtype=torch.bool, device=dev) if mask is None else mask.clone()
        mask[b[:, 0]] = True
        mask[b[:, 1]] = True
    return None if mask is None else mask.to(torch.uint8).contiguous()


def _laplace_step(d, pos, out, step):
    d.pos, d.sm_pos_out, d.sm_step = ptr(pos), ptr(out), step
    call("nudf_meshsmooth_laplace", d)
    return out


def smooth_mesh(verts, faces, iterations=10, lam=0.5, mu=-0.53, weights="uniform", boundary="fixed", fixed=None):
    """Laplacian smoothing of the whole mesh, by default Taubin's lambda | mu scheme -> verts' [V, 3] in the input's dtype
    (csrc/meshsmooth.hip; trimesh.smoothing.filter_taubin and open3d's filter_smooth_taubin on the CPU).  Each of
    `iterations` rounds is a Jacobi step p + lam (m - p) and, unless mu = 0, a second one with mu (negative: it undoes the
    shrinkage of the first; mu = 0 is plain Laplacian smoothing), every step from the positions of the one before.
    weights="uniform": m is the mean of the one-ring (vertex_adjacency), summed in ascending index.  "cotangent": m is
    the mean weighted by max(cot, 0) / 2 of the angles opposite each edge, summed over the vertex's corners in ascending
    3 f + k from the positions of the current step; a face of zero area adds nothing.  boundary="fixed" keeps the ends of
    the edges with exactly one face where they are, "free" lets them move (an open surface then shrinks at its border);
    `fixed` [V] marks further vertices to keep.  A vertex without neighbours, or with cotangent weights one whose faces
    are all degenerate, stays.  float64 inside, cast at the end; identical from run to run.  An empty mesh and
    iterations = 0 return the input."""
    iterations = _count(iterations, "iterations")
    lam, mu = _finite(lam, "lam"), _finite(mu, "mu")
    if weights not in ("uniform", "cotangent"):
        raise ValueError(f"weights must be 'uniform' or 'cotangent' (got {weights!r})")
    verts, faces = _check_mesh(verts, faces)
    n_verts, n_faces = verts.shape[0], faces.shape[0]
    table = _mesh_edges(faces, n_verts) if n_faces and n_verts and (weights == "uniform" or boundary == "fixed") else None
    mask = _fixed_mask(verts, table, boundary, fixed)
    if n_faces == 0 or n_verts == 0 or iterations == 0:
        return verts
    d = _lib.MeshOrient(faces=ptr(faces), n_faces=n_faces, n_verts=n_verts, sm_fixed=ptr(mask),
                        sm_weights=0 if weights == "uniform" else 1)
    if weights == "uniform":
        nbr_off, nbr = _vertex_adjacency(faces, n_verts, table)
        d.sm_nbr_off, d.sm_nbr, d.sm_n_nbr = ptr(nbr_off), ptr(nbr), nbr.numel()
    else:
        corner_off, corner = _corner_lists(faces, n_verts)
        d.corner_off, d.corner = ptr(corner_off), ptr(corner)
    pos = verts.double().contiguous()                # may be the caller's tensor: read only
    bufs = [torch.empty_like(pos), torch.empty_like(pos)]
    n = 0
    for _ in range(iterations):
        for step in (lam, mu) if mu != 0 else (lam,):
            pos = _laplace_step(d, pos, bufs[n % 2], step)
            n += 1
    return pos.to(verts.dtype)


def _mean_edge_length(pos, table):
    """numpy's mean of the float64 lengths of the unique edges (u != v) in the table's order; one copy to the host, so that
    the value does not depend on the order of a reduction on the GPU"""
    e = table.edges
    e = e[e[:, 0] != e[:, 1]]
    d = pos[e[:, 0]] - pos[e[:, 1]]
    d2 = d * d
    length = torch.sqrt((d2[:, 0] + d2[:, 1]) + d2[:, 2])
    return float(np.mean(length.cpu().numpy())) if length.numel() else math.nan


def _face_frames(d, n_faces, dev):
    """launches frames -> (normals [F, 3], areas [F], centres [F, 3]) float64; d must hold faces and pos"""
    fnormal = torch.empty((n_faces, 3), dtype=torch.float64, device=dev)
    area = torch.empty(n_faces, dtype=torch.float64, device=dev)
    centre = torch.empty((n_faces, 3), dtype=torch.float64, device=dev)
    d.sm_fnormal_out, d.sm_farea, d.sm_fcentre = ptr(fnormal), ptr(area), ptr(centre)
    call("nudf_meshsmooth_frames", d)
    return fnormal, area, centre


def denoise_mesh(verts, faces, normal_iterations=5, vertex_iterations=10, sigma_s=0.35, sigma_c=None, boundary="fixed",
                 fixed=None):
    """feature-preserving denoising: a bilateral filter on the face normals, then the vertices moved to fit them
    -> (verts' [V, 3], face normals [F, 3]), both in the input's dtype (csrc/meshsmooth.hip; Zheng et al. 2011, "Bilateral
    normal filtering for mesh denoising", with the vertex update of Sun et al. 2007).  The normals, areas and centres of
    the faces are taken once from the input.  Each of `normal_iterations` steps replaces the normal of face i by the
    normalised sum, over the faces j that share a vertex with i, of area_j exp(-|c_i - c_j|^2 / (2 sigma_c^2)
    - |n_i - n_j'|^2 / (2 sigma_s^2)) n_j', where n_j' is n_j turned into the half-space of n_i: the mesher's faces are not
    consistently wound, and without the turn neighbours of opposite winding would cancel.  The returned normals keep the
    side of the input's faces.  sigma_c = None: the mean length of the unique edges.  Each of `vertex_iterations` Jacobi
    steps then moves a vertex by the mean over its faces of n_f (n_f . (c_f - p)), c_f the current centre of the face.
    `boundary` and `fixed` as in smooth_mesh; a vertex whose faces all have zero area stays, a face of zero area has the
    normal (0, 0, 0) and takes no part.  The neighbours of a face are visited through its vertices in ascending index, so
    the result does not depend on the winding: flipping faces leaves the positions bit for bit and the normals up to
    sign.  float64 inside, cast at the end; identical from run to run.  An empty mesh returns the input and no normals."""
    normal_iterations = _count(normal_iterations, "normal_iterations")
    vertex_iterations = _count(vertex_iterations, "vertex_iterations")
    sigma_s = _finite(sigma_s, "sigma_s", positive=True)
    if sigma_c is not None:
        sigma_c = _finite(sigma_c, "sigma_c", positive=True)
    verts, faces = _check_mesh(verts, faces)
    n_verts, n_faces, dev = verts.shape[0], faces.shape[0], verts.device
    table = None
    if n_faces and n_verts and (boundary == "fixed" or (sigma_c is None and normal_iterations)):
        table = _mesh_edges(faces, n_verts)
    mask = _fixed_mask(verts, table, boundary, fixed)
    if n_faces == 0 or n_verts == 0:
        return verts, torch.zeros((n_faces, 3), dtype=verts.dtype, device=dev)
    pos = verts.double().contiguous()                # may be the caller's tensor: read only
    corner_off, corner = _corner_lists(faces, n_verts)
    d = _lib.MeshOrient(faces=ptr(faces), pos=ptr(pos), corner_off=ptr(corner_off), corner=ptr(corner), n_faces=n_faces,
                        n_verts=n_verts, sm_fixed=ptr(mask))
    fnormal, area, centre = _face_frames(d, n_faces, dev)
    if normal_iterations:
        if sigma_c is None:
            sigma_c = _mean_edge_length(pos, table)
            if not (sigma_c > 0 and math.isfinite(sigma_c)):
                raise ValueError(f"the mean edge length {sigma_c} is not positive and finite: give sigma_c")
        d.sm_inv2sc, d.sm_inv2ss = 1.0 / (2.0 * sigma_c * sigma_c), 1.0 / (2.0 * sigma_s * sigma_s)
        other = torch.empty_like(fnormal)
        for _ in range(normal_iterations):
            d.sm_fnormal, d.sm_fnormal_out = ptr(fnormal), ptr(other)
            call("nudf_meshsmooth_normals", d)
            fnormal, other = other, fnormal
    d.sm_fnormal = ptr(fnormal)
    bufs = [torch.empty_like(pos), torch.empty_like(pos)] if vertex_iterations else []
    for i in range(vertex_iterations):
        d.pos, d.sm_pos_out = ptr(pos), ptr(bufs[i % 2])
        call("nudf_meshsmooth_update", d)
        pos = bufs[i % 2]
    return pos.to(verts.dtype), fnormal.to(verts.dtype)


def compact_mesh(verts, faces, vertex_mask=None, face_mask=None, drop_unreferenced=True):
    """drops the faces outside `face_mask` and those with a vertex outside `vertex_mask`, then the vertices outside
    `vertex_mask` and, with drop_unreferenced, those no remaining face uses; the survivors keep their order
    -> (verts', faces' into them)"""
    if vertex_mask is not None and faces.numel():
        keep = vertex_mask[faces].all(1)
        face_mask = keep if face_mask is None else face_mask & keep
    if face_mask is not None:
        faces = faces[face_mask]
    keep = vertex_mask
    if drop_unreferenced:
        keep = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
        keep[faces.reshape(-1)] = True
    if keep is None:
        return verts, faces
    remap = torch.cumsum(keep, 0) - 1
    return verts[keep], remap[faces]


def filter_components(verts, faces, min_faces=500, keep_largest=False):
    """keeps the components (face_components) with at least min_faces faces, or with keep_largest the largest one only
    (tie: the one with the smallest face index), and drops the vertices no kept face uses -> (verts', faces')
    (clean_dtu_mesh.py clean_mesh_by_faces_num and clean_outliers(keep_largest=True))"""
    verts, faces = _check_mesh(verts, faces)
    if faces.shape[0] == 0:
        return verts, faces
    labels = face_components(faces, verts.shape[0])
    size = torch.bincount(labels, minlength=faces.shape[0])
    if keep_largest:
        mask = labels == torch.nonzero(size == size.max())[0, 0]                  # first index of the maximum
    else:
        mask = size[labels] >= int(min_faces)
    return compact_mesh(verts, faces, face_mask=mask)


class Simplified(NamedTuple):
    """verts [V', 3] in the input's dtype; faces [F', 3] int64 into them; vertex_cluster [V] int64: the output vertex of
    each input vertex, -1 where its cluster was dropped; face_src [F'] int64: the input face of each output face,
    ascending; accepted [V'] bool: the vertex is the quadric's minimiser (otherwise its cluster's mean); attributes
    [V', k] in their input's dtype, or None"""
    verts: torch.Tensor
    faces: torch.Tensor
    vertex_cluster: torch.Tensor
    face_src: torch.Tensor
    accepted: torch.Tensor
    attributes: torch.Tensor | None


def _three_finite(x, name):
    try:
        o = [float(t) for t in x]
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three finite numbers (got {x!r})") from None
    if len(o) != 3 or not all(math.isfinite(t) for t in o):
        raise ValueError(f"{name} must be three finite numbers (got {x!r})")
    return o


def _simplify_grid(pos, cell, origin):
    """`cell` and `origin` against the vertices -> (cell, origin [3], cells per axis [3]); one read-back of the bounds"""
    try:
        cell = float(cell)
    except (TypeError, ValueError):
        raise ValueError(f"cell must be a positive finite number (got {cell!r})") from None
    if not (cell > 0 and math.isfinite(cell)):
        raise ValueError(f"cell must be a positive finite number (got {cell!r})")
    lo, hi = torch.stack(torch.aminmax(pos, dim=0)).tolist()
    if not all(math.isfinite(x) for x in lo + hi):
        raise ValueError("a vertex is not finite")
    if origin is None:
        origin = lo
    else:
        origin = _three_finite(origin.tolist() if isinstance(origin, torch.Tensor) else origin, "origin")
        if any(o > m for o, m in zip(origin, lo)):
            raise ValueError(f"origin {origin} lies above the vertices' minimum {lo}")
    grid = []
    for o, m in zip(origin, hi):
        q = (m - o) / cell                                   # floor is monotone: the largest vertex has the largest cell
        if not q < SIMPLIFY_MAX_GRID:
            raise ValueError(f"cell {cell} gives more than 2^20 cells along an axis (extent {m - o})")
        grid.append(int(math.floor(q)) + 1)
    return cell, origin, grid


def _simplify_desc(pos, faces, cell, origin, grid):
    d = _topo(faces, pos.shape[0])
    d.pos, d.sp_cell = ptr(pos), cell
    for x in range(3):
        d.sp_origin[x], d.sp_grid[x] = origin[x], grid[x]
    return d


def _stage(events, state, name):
    """ends the open stage and starts `name` (None: ends the last one); nothing without an event dict"""
    if events is None:
        return
    if "open" in state:
        events[state["open"]][1].record()
    if name is not None:
        events[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        events[name][0].record()
        state["open"] = name
    else:
        state.pop("open", None)


def _vertex_clusters(d, n_verts, dev, events=None, state=None):
    """rules 1 and 2 for the vertices -> (cluster_key [C] ascending, vcluster [V], member [V]: the vertices by cluster,
    ascending inside each, member_off [C + 1]).  d keeps pointers into the four: the caller holds them."""
    keys = torch.empty(n_verts, dtype=torch.int64, device=dev)
    d.sp_key = ptr(keys)
    _stage(events, state, "keys")
    call("nudf_meshsimplify_keys", d)
    _stage(events, state, "sorts")
    skey, member = torch.sort(keys, stable=True)
    if int(skey[0]) < 0:
        raise ValueError("a vertex is not finite or lies outside the grid")
    first = torch.ones(n_verts, dtype=torch.bool, device=dev)
    first[1:] = skey[1:] != skey[:-1]
    start = torch.nonzero(first).reshape(-1)
    vcluster = torch.empty(n_verts, dtype=torch.int64, device=dev)
    vcluster[member] = torch.cumsum(first, 0) - 1
    member_off = torch.cat([start, torch.full((1,), n_verts, dtype=torch.int64, device=dev)])
    return skey[start].contiguous(), vcluster, member.contiguous(), member_off


def _surviving_faces(d, faces, vcluster, n_clusters, events=None, state=None):
    """rule 5 up to the compaction -> (the surviving faces over cluster ids, their source indices ascending)"""
    n, dev = faces.shape[0], faces.device
    out = torch.empty((n, 3), dtype=torch.int64, device=dev)
    triple = torch.empty((n, 3), dtype=torch.int64, device=dev)
    degenerate = torch.empty(n, dtype=torch.uint8, device=dev)
    d.sp_vcluster, d.sp_faces, d.sp_triple, d.sp_degenerate = ptr(vcluster), ptr(out), ptr(triple), ptr(degenerate)
    d.n_clusters = n_clusters
    _stage(events, state, "faces")
    call("nudf_meshsimplify_faces", d)
    _stage(events, state, "dedupe")
    src = torch.nonzero(degenerate == 0).reshape(-1)
    t = triple[src]
    # by (a, b, c), equal triples by source index: two stable sorts, the less significant key first (a C + b < 2^62)
    order = torch.sort(t[:, 2], stable=True).indices
    order = order[torch.sort((t[:, 0] * n_clusters + t[:, 1])[order], stable=True).indices]
    ts = t[order]
    first = torch.ones(order.numel(), dtype=torch.bool, device=dev)
    first[1:] = (ts[1:] != ts[:-1]).any(1)
    keep = torch.sort(src[order[first]]).values
    return out[keep], keep


def _check_attributes(attributes, verts):
    if attributes is None:
        return None
    if not isinstance(attributes, torch.Tensor) or not attributes.is_floating_point():
        raise ValueError("attributes must be a floating-point torch tensor")
    if attributes.dim() != 2 or attributes.shape[0] != verts.shape[0]:
        raise ValueError(f"attributes must be [{verts.shape[0]}, k] (got {tuple(attributes.shape)})")
    if attributes.device != verts.device:
        raise ValueError(f"attributes must be on the vertices' GPU (got {attributes.device})")
    return attributes


def simplify_mesh(verts, faces, cell, origin=None, boundary_weight=1.0, regularisation=1e-3, placement="quadric",
                  attributes=None, _info=None, measure=False):
    """vertex clustering on a uniform grid of edge `cell`, each cluster's vertex placed by quadric error minimisation
    (csrc/meshsimplify.hip) -> Simplified(verts, faces, vertex_cluster, face_src, accepted, attributes).
    1. Keys: c = floor((p - origin) / cell) per axis in float64, key = (cx Gy + cy) Gz + cz with G = max c + 1 <= 2^20 per
       axis.  `origin` defaults to the vertices' minimum; a given one must not lie above it.  A flat part of the mesh that
       lies exactly at the minimum sits on a cell wall, where the accept test of step 4 hangs on the last bit: an origin a
       fraction of a cell lower avoids that.
    2. Clusters are the unique keys in ascending order, with their vertices and their corners 3 f + k in ascending order.
    3. Quadric of a cluster, local to its cell's centre origin + (c + 1/2) cell, summed over its corners in that order in
       float64: corner (f, k) adds the plane of f with weight |n| / 2 (n = (p1 - p0) x (p2 - p0); a face of zero or
       non-finite |n| adds nothing, a face with two corners in the cluster adds twice) and, for the half-edge that starts
       at the corner and for the one that ends there, when it is a boundary half-edge (its edge has one face in the
       EdgeTable), the plane through the edge that stands on the face, with boundary_weight times the face's weight.
       Without them an open surface shrinks at its border; boundary_weight = 0 leaves them out.
    4. Placement: with t = tr(A) > 0, x solves (A + lambda t I) x = -b + lambda t mean (lambda = regularisation, mean = that
       of the cluster's vertices; a 3 x 3 Cholesky factorisation, the condition is at most (1 + lambda) / lambda) and is
       taken exactly when centre + x has the cluster's key; otherwise, and always with placement="mean", the vertex is
       the mean.  Every output vertex lies in its cluster's cell.
    5. Faces: corners become cluster ids; a face that repeats an id goes; of the faces with the same three ids, whatever
       the winding, the one with the smallest index stays; survivors keep their order and corner order; clusters that no
       face uses are dropped.
    6. `attributes` [V, k] (colours, normals): the mean over each cluster's vertices, float64 inside.
    Unlike open3d's simplify_vertex_clustering (quadric mode): boundary quadrics, a regularised solve in place of a
    pseudo-inverse, and a solution outside its cell is refused.  Stable sorts and scans in torch between three launches,
    sums in list order without atomics: identical from run to run.  (`_info`: a dict that receives clusters, grid, origin,
    cell, fallbacks and quadric [V', 10] = A00 A01 A02 A11 A12 A22 b0 b1 b2 c of each output vertex; when it holds a dict
    under "events", that receives a pair of events per stage.)
    With measure=True the result's two-sided deviation from the input is measured (evaluation.mesh_deviation, vertices
    only) and returned beside it: -> (Simplified, deviation); `_info` receives it too, under "deviation".  Off by
    default: the result and its cost are then exactly as without the argument."""
    if placement not in ("quadric", "mean"):
        raise ValueError(f"placement must be 'quadric' or 'mean' (got {placement!r})")
    try:
        boundary_weight, regularisation = float(boundary_weight), float(regularisation)
    except (TypeError, ValueError):
        raise ValueError("boundary_weight and regularisation must be numbers") from None
    if not (boundary_weight >= 0 and math.isfinite(boundary_weight)):
        raise ValueError(f"boundary_weight must be >= 0 and finite (got {boundary_weight})")
    if not (regularisation > 0 and math.isfinite(regularisation)):
        raise ValueError(f"regularisation must be > 0 and finite (got {regularisation})")
    verts, faces = _check_mesh(verts, faces)
    attributes = _check_attributes(attributes, verts)
    n_verts, n_faces, dev = verts.shape[0], faces.shape[0], verts.device
    if n_verts == 0 or n_faces == 0:
        try:
            cell = float(cell)
        except (TypeError, ValueError):
            cell = math.nan
        if not (cell > 0 and math.isfinite(cell)):
            raise ValueError(f"cell must be a positive finite number (got {cell!r})")
        if _info is not None:
            _info.update(clusters=0, grid=[0, 0, 0], origin=None, cell=cell, fallbacks=0,
                         quadric=torch.zeros((0, 10), dtype=torch.float64, device=dev))
        out = Simplified(verts[:0], faces[:0], torch.full((n_verts,), -1, dtype=torch.int64, device=dev),
                         torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.bool, device=dev),
                         None if attributes is None else attributes[:0])
        if measure:
            raise ValueError("measure=True needs a mesh with faces")
        return out
    events, state = None if _info is None else _info.get("events"), {}
    pos = verts.double().contiguous()
    cell, origin, grid = _simplify_grid(pos, cell, origin)
    d = _simplify_desc(pos, faces, cell, origin, grid)
    cluster_key, vcluster, member, member_off = _vertex_clusters(d, n_verts, dev, events, state)
    n_clusters = cluster_key.numel()
    d.n_clusters = n_clusters
    quadric_rule = placement == "quadric"
    table = corner = corner_off = None
    if quadric_rule:
        ckey = vcluster[faces.reshape(-1)]
        corner = torch.sort(ckey, stable=True).indices                   # corners 3 f + k by cluster, ascending inside
        corner_off = torch.zeros(n_clusters + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(ckey, minlength=n_clusters), 0, out=corner_off[1:])
        del ckey
        if boundary_weight != 0:
            table = _mesh_edges(faces, n_verts)
            d.edges, d.he_edge, d.n_edges = ptr(table.edges), ptr(table.he_edge), table.edges.shape[0]
    _stage(events, state, "place")
    rep = torch.empty((n_clusters, 3), dtype=torch.float64, device=dev)
    accepted = torch.empty(n_clusters, dtype=torch.uint8, device=dev)
    quadric = torch.zeros((n_clusters, 10), dtype=torch.float64, device=dev) if _info is not None else None
    attr = attr_out = None
    if attributes is not None and attributes.shape[1]:
        attr = attributes.double().contiguous()
        attr_out = torch.empty((n_clusters, attr.shape[1]), dtype=torch.float64, device=dev)
        d.sp_attr, d.sp_attr_out, d.sp_attr_width = ptr(attr), ptr(attr_out), attr.shape[1]
    d.sp_cluster_key, d.sp_member_off, d.sp_member = ptr(cluster_key), ptr(member_off), ptr(member)
    d.sp_corner_off, d.sp_corner = ptr(corner_off), ptr(corner)
    d.sp_rep, d.sp_accepted, d.sp_quadric = ptr(rep), ptr(accepted), ptr(quadric)
    d.sp_lambda, d.sp_boundary_weight, d.sp_placement = regularisation, boundary_weight, 0 if quadric_rule else 1
    call("nudf_meshsimplify_place", d)
    new_faces, face_src = _surviving_faces(d, faces, vcluster, n_clusters, events, state)
    _stage(events, state, "compact")
    kept, out_faces = compact_mesh(torch.arange(n_clusters, dtype=torch.int64, device=dev), new_faces)
    remap = torch.full((n_clusters,), -1, dtype=torch.int64, device=dev)
    remap[kept] = torch.arange(kept.numel(), dtype=torch.int64, device=dev)
    out_attr = None
    if attributes is not None:
        out_attr = attributes.new_zeros((kept.numel(), 0)) if attr_out is None else attr_out[kept].to(attributes.dtype)
    out = Simplified(rep[kept].to(verts.dtype), out_faces, remap[vcluster], face_src, accepted[kept].bool(), out_attr)
    _stage(events, state, None)
    if _info is not None:
        _info.update(clusters=n_clusters, grid=grid, origin=origin, cell=cell, quadric=quadric[kept],
                     fallbacks=int((~out.accepted).sum()) if quadric_rule else 0)
    if measure:
        deviation = _deviation(pos, faces, out)
        if _info is not None:
            _info["deviation"] = deviation
        return out, deviation
    return out


def _count_faces(pos, faces, cell, origin):
    """the number of faces simplify_mesh would leave with this cell: keys, unique, remap, dedupe; no quadrics"""
    cell, origin, grid = _simplify_grid(pos, cell, origin)
    d = _simplify_desc(pos, faces, cell, origin, grid)
    cluster_key, vcluster, _, _ = _vertex_clusters(d, pos.shape[0], pos.device)
    return _surviving_faces(d, faces, vcluster, cluster_key.numel())[1].numel()


def simplify_to_faces(verts, faces, target_faces, **kw):
    """simplify_mesh with the finest grid a bisection finds that leaves at most `target_faces` faces -> Simplified.  The
    grid has n cells along the longest side of the bounding box (cell = side / n, a hair more so that the largest vertex
    does not open a cell of its own) and starts at the box's minimum; n is bisected over [1, min(2^20 - 1, V)] in at most
    24 rounds, each a count-only pass (keys, unique, remap, dedupe).  The result is guaranteed to have at most
    target_faces faces; it is not guaranteed to be the largest such result, because the count is not strictly monotone in
    n.  With target_faces >= F the input comes back unchanged (accepted all False).  Further arguments go to
    simplify_mesh (`cell` and `origin` are the search's own)."""
    if "cell" in kw or "origin" in kw:
        raise ValueError("simplify_to_faces chooses cell and origin itself")
    try:
        target = int(target_faces)
    except (TypeError, ValueError):
        raise ValueError(f"target_faces must be an integer >= 0 (got {target_faces!r})") from None
    if target < 0 or target != target_faces:
        raise ValueError(f"target_faces must be an integer >= 0 (got {target_faces!r})")
    verts, faces = _check_mesh(verts, faces)
    attributes = _check_attributes(kw.get("attributes"), verts)
    n_verts, n_faces, dev = verts.shape[0], faces.shape[0], verts.device
    if n_faces == 0 or n_verts == 0:
        return simplify_mesh(verts, faces, 1.0, **kw)
    if n_faces <= target:
        return Simplified(verts, faces, torch.arange(n_verts, dtype=torch.int64, device=dev),
                          torch.arange(n_faces, dtype=torch.int64, device=dev),
                          torch.zeros(n_verts, dtype=torch.bool, device=dev), attributes)
    pos = verts.double().contiguous()
    lo, hi = torch.stack(torch.aminmax(pos, dim=0)).tolist()
    if not all(math.isfinite(x) for x in lo + hi):
        raise ValueError("a vertex is not finite")
    side = max(h - l for l, h in zip(lo, hi))
    side = side if side > 0 else 1.0

    def cell_of(n):
        return side / n * (1.0 + 1e-9)
    n_lo, n_hi = 1, min(SIMPLIFY_MAX_GRID - 1, max(1, n_verts))
    for _ in range(SIMPLIFY_BISECT_ROUNDS):
        if n_lo >= n_hi:
            break
        mid = (n_lo + n_hi + 1) // 2
        if _count_faces(pos, faces, cell_of(mid), lo) <= target:
            n_lo = mid
        else:
            n_hi = mid - 1
    return simplify_mesh(verts, faces, cell_of(n_lo), origin=lo, **kw)


def _deviation(src, src_faces, result):
    """mesh_deviation(input, result), vertices only; `src`: (vertices, faces) or the input's MeshIndex.  A result without
    faces is infinitely far"""
    from . import evaluation                                 # lazily: evaluation imports meshing, which imports this file
    if result.faces.shape[0] == 0:
        inf = dict(max=math.inf, mean=math.inf, rms=math.inf, n=0)
        return dict(a_to_b=inf, b_to_a=dict(inf), hausdorff=math.inf)
    a = src if isinstance(src, evaluation.MeshIndex) else (src, src_faces)
    return evaluation.mesh_deviation(a, (result.verts.double(), result.faces))


def simplify_to_error(verts, faces, max_error, **kw):
    """simplify_mesh on the coarsest grid a bisection finds whose measured deviation from the input is at most
    `max_error` -> (Simplified, deviation).  The deviation is evaluation.mesh_deviation(input, result)["hausdorff"],
    vertices only: the exact distance from every input vertex to the result's surface and from every result vertex to the
    input's, the larger of the two maxima (a lower bound of the true Hausdorff distance, exact at the vertices).  The grid
    has n cells along the longest side of the bounding box, as in simplify_to_faces; n is bisected over
    [1, min(2^20 - 1, V)] in at most 24 passes, each a full simplification and measurement (the input's MeshIndex is
    built once, the result's per pass).  The deviation is not monotone in n, so the result meets the bound but need not
    be the coarsest grid that does.  When no grid tried meets it the input comes back unchanged: vertex_cluster and
    face_src are arange, accepted is all True, the deviation is 0 in every figure.  Further arguments go to simplify_mesh
    (`cell`, `origin` and `measure` are the search's own)."""
    if "cell" in kw or "origin" in kw or "measure" in kw:
        raise ValueError("simplify_to_error chooses cell and origin itself and always measures")
    try:
        max_error = float(max_error)
    except (TypeError, ValueError):
        raise ValueError(f"max_error must be a number >= 0 (got {max_error!r})") from None
    if not max_error >= 0:
        raise ValueError(f"max_error must be a number >= 0 (got {max_error!r})")
    from . import evaluation
    verts, faces = _check_mesh(verts, faces)
    attributes = _check_attributes(kw.get("attributes"), verts)
    n_verts, n_faces, dev = verts.shape[0], faces.shape[0], verts.device
    if n_faces == 0 or n_verts == 0:
        raise ValueError("simplify_to_error needs a mesh with faces")
    pos = verts.double().contiguous()
    lo, hi = torch.stack(torch.aminmax(pos, dim=0)).tolist()
    if not all(math.isfinite(x) for x in lo + hi):
        raise ValueError("a vertex is not finite")
    side = max(h - l for l, h in zip(lo, hi))
    side = side if side > 0 else 1.0
    index = evaluation.MeshIndex(pos, faces)
    best = None
    n_lo, n_hi = 1, min(SIMPLIFY_MAX_GRID - 1, max(1, n_verts))
    for _ in range(SIMPLIFY_BISECT_ROUNDS):
        if n_lo > n_hi:
            break
        mid = (n_lo + n_hi) // 2
        s = simplify_mesh(verts, faces, side / mid * (1.0 + 1e-9), origin=lo, **kw)
        deviation = _deviation(index, None, s)
        if deviation["hausdorff"] <= max_error:
            best, n_hi = (s, deviation), mid - 1                # met: look for a coarser grid
        else:
            n_lo = mid + 1
    if best is not None:
        return best
    zero = dict(max=0.0, mean=0.0, rms=0.0, n=n_verts)
    same = Simplified(verts, faces, torch.arange(n_verts, dtype=torch.int64, device=dev),
                      torch.arange(n_faces, dtype=torch.int64, device=dev),
                      torch.ones(n_verts, dtype=torch.bool, device=dev), attributes)
    return same, dict(a_to_b=zero, b_to_a=dict(zero), hausdorff=0.0)


def transfer_attributes(src_verts, src_faces, src_attributes, dst_points, bound=math.inf):
    """attributes of a mesh at the places of it that lie closest to `dst_points` [M, 3]: for each point the closest
    point of the source surface (evaluation.closest_on_mesh, exact) and there the barycentric blend
    (w0 a0 + w1 a1) + w2 a2 of the three attribute rows of its face, in float64 -> [M, k] in the attributes' dtype.
    src_attributes [V, k] floating point (colours, normals, any per-vertex quantity).  Rows farther than `bound` from the
    source are NaN.  Carries what simplify_mesh only averages, and after any other edit of the mesh."""
    from . import evaluation
    if not isinstance(src_attributes, torch.Tensor) or not src_attributes.is_floating_point() or src_attributes.dim() != 2:
        raise ValueError("src_attributes must be a floating-point [V, k] torch tensor")
    index = evaluation.MeshIndex(src_verts, src_faces)
    if src_attributes.shape[0] != index.vertices.shape[0]:
        raise ValueError(f"src_attributes must be [{index.vertices.shape[0]}, k] (got {tuple(src_attributes.shape)})")
    c = index.closest(dst_points, bound)
    a = src_attributes.to(device=index.vertices.device, dtype=torch.float64)
    hit = c.face >= 0
    rows = a[index.faces[c.face.clamp(min=0)]]                                  # [M, 3, k]
    w = c.bary.unsqueeze(2)
    out = (w[:, 0] * rows[:, 0] + w[:, 1] * rows[:, 1]) + w[:, 2] * rows[:, 2]
    out[~hit] = math.nan
    return out.to(src_attributes.dtype)


class Subdivided(NamedTuple):
    """verts [V', 3] in the input's dtype, the first V rows being the input's vertices; faces [F', 3] int64; attributes
    [V', k] in their input's dtype, or None; parent_face [F'] int64: the input face each output face lies in; rounds: the
    rounds that split an edge; longest_edge: the float64 length of the result's longest edge; converged: False only when
    subdivide_to_edge stopped at max_rounds with edges above the bound left"""
    verts: torch.Tensor
    faces: torch.Tensor
    attributes: torch.Tensor | None
    parent_face: torch.Tensor
    rounds: int
    longest_edge: float
    converged: bool


_SUBDIVIDE_SCHEMES = {"midpoint": 0, "loop": 1}


def _longest_edge(pos, table):
    """the float64 length of the longest edge with two different ends, 0.0 without one: the maximum of
    (dx dx + dy dy) + dz dz on the GPU (a maximum does not depend on its order) and one square root on the host"""
    e = table.edges
    e = e[e[:, 0] != e[:, 1]]
    if e.shape[0] == 0:
        return 0.0
    d = pos[e[:, 0]] - pos[e[:, 1]]
    d2 = d * d
    return math.sqrt(float(((d2[:, 0] + d2[:, 1]) + d2[:, 2]).max()))


def _loop_classes(table, boundary, n_verts):
    """-> uint8 [V]: 2 (stays) for the ends of an edge with three or more half-edges and for a vertex whose number of
    border edges is neither 0 nor 2, 1 (border) for one with two border edges, 0 (smooth) otherwise"""
    e = table.edges
    bdeg = boundary.nbr_off[1:] - boundary.nbr_off[:-1]
    vclass = torch.zeros(n_verts, dtype=torch.uint8, device=e.device)
    vclass[bdeg == 2] = 1
    vclass[(bdeg != 0) & (bdeg != 2)] = 2
    multi = e[e[:, 2] >= 3]
    vclass[multi[:, 0]] = 2
    vclass[multi[:, 1]] = 2
    return vclass


def _subdivide_round(pos, faces, attr, scheme, max_edge, split=True, events=None, state=None):
    """one round on float64 positions (and attributes or None): marks every edge (max_edge None) or those longer than
    max_edge and, with `split`, splits them -> (edges marked, pos', faces', attr', parent, table); faces' is None when
    nothing was split, and `table` is the input's EdgeTable"""
    n_verts, n_faces, dev = pos.shape[0], faces.shape[0], pos.device
    _stage(events, state, "edges")
    table = _mesh_edges(faces, n_verts)
    n_edges = table.edges.shape[0]
    d = _topo(faces, n_verts, table)
    d.pos = ptr(pos)
    _stage(events, state, "mark")
    mark = torch.empty(n_edges, dtype=torch.uint8, device=dev)
    d.sp_sd_mark, d.sp_sd_mark_all, d.sp_sd_max_edge = ptr(mark), int(max_edge is None), 0.0 if max_edge is None else max_edge
    call("nudf_meshsubdiv_mark", d)
    marked = torch.nonzero(mark).reshape(-1)
    n_marked = marked.numel()
    if n_marked == 0 or not split:
        _stage(events, state, None)
        return n_marked, pos, None, attr, None, table
    if n_verts + n_marked >= MAX_VERTS:
        raise ValueError(f"{n_verts} vertices and {n_marked} split edges: the result would have 2^31 vertices or more")
    rank = torch.cumsum(mark, 0, dtype=torch.int64)
    edge_vertex = torch.where(mark != 0, rank + (n_verts - 1), torch.full_like(rank, -1))
    d.sp_sd_marked, d.sp_sd_edge_vertex, d.sp_sd_n_marked, d.sp_sd_scheme = ptr(marked), ptr(edge_vertex), n_marked, scheme
    pos_out = torch.empty((n_verts + n_marked, 3), dtype=torch.float64, device=dev)
    d.sp_sd_pos_out = ptr(pos_out)
    attr_out = None
    if attr is not None:
        attr_out = torch.empty((n_verts + n_marked, attr.shape[1]), dtype=torch.float64, device=dev)
        if attr.shape[1]:
            d.sp_attr, d.sp_sd_attr_out, d.sp_attr_width = ptr(attr), ptr(attr_out), attr.shape[1]
    if scheme == 1:
        _stage(events, state, "adjacency")
        ring_off, ring = _vertex_adjacency(faces, n_verts, table)
        boundary = _boundary(table, n_verts)
        vclass = _loop_classes(table, boundary, n_verts)
        d.sp_sd_ring_off, d.sp_sd_ring, d.sp_sd_n_ring = ptr(ring_off), ptr(ring), ring.numel()
        d.nbr_off, d.nbr, d.sp_sd_n_border = ptr(boundary.nbr_off), ptr(boundary.nbr), boundary.nbr.numel()
        d.sp_sd_vclass = ptr(vclass)
    _stage(events, state, "vertices")
    call("nudf_meshsubdiv_odd", d)
    call("nudf_meshsubdiv_even", d)
    _stage(events, state, "faces")
    fcount = torch.empty(n_faces, dtype=torch.int64, device=dev)
    d.sp_sd_fcount = ptr(fcount)
    call("nudf_meshsubdiv_count", d)
    fend = torch.cumsum(fcount, 0)
    foff = fend - fcount
    n_out = int(fend[-1])
    faces_out = torch.empty((n_out, 3), dtype=torch.int64, device=dev)
    parent = torch.empty(n_out, dtype=torch.int64, device=dev)
    d.sp_sd_foff, d.sp_sd_faces_out, d.sp_sd_parent, d.sp_sd_n_out = ptr(foff), ptr(faces_out), ptr(parent), n_out
    call("nudf_meshsubdiv_emit", d)
    _stage(events, state, None)
    return n_marked, pos_out, faces_out, attr_out, parent, table


def _subdivide(verts, faces, attributes, scheme, max_edge, rounds_cap, _info):
    """the rounds of both drivers: `rounds_cap` rounds of `scheme` on every edge (max_edge None), or rounds of midpoint
    splits of the edges above max_edge until none is left or the cap is reached"""
    verts, faces = _check_mesh(verts, faces)
    attributes = _check_attributes(attributes, verts)
    n_faces, dev = faces.shape[0], verts.device
    parent = torch.arange(n_faces, dtype=torch.int64, device=dev)
    if verts.shape[0] == 0 or n_faces == 0:
        return Subdivided(verts, faces, attributes, parent, 0, 0.0, True)
    events = None if _info is None else _info.get("events")
    pos = verts.double().contiguous()                    # may be the caller's tensor: read only
    attr = None if attributes is None else attributes.double().contiguous()
    out_faces, rounds, converged, table = faces, 0, True, None
    while max_edge is not None or rounds < rounds_cap:
        stages = None if events is None else events.setdefault(f"round{rounds}", {})
        n_marked, new_pos, new_faces, new_attr, new_parent, table = _subdivide_round(
            pos, out_faces, attr, scheme, max_edge, rounds < rounds_cap, stages, {})
        if new_faces is None:                            # nothing to split, or the cap: only the marks were looked at
            converged = n_marked == 0
            break
        pos, out_faces, attr, parent, rounds, table = new_pos, new_faces, new_attr, parent[new_parent], rounds + 1, None
    if table is None:
        table = _mesh_edges(out_faces, pos.shape[0])
    return Subdivided(pos.to(verts.dtype), out_faces, None if attributes is None else attr.to(attributes.dtype), parent,
                      rounds, _longest_edge(pos, table), converged)


def subdivide_mesh(verts, faces, levels=1, scheme="loop", attributes=None, _info=None):
    """uniform subdivision, `levels` times, each level from the one before (csrc/meshsubdiv.hip; trimesh.remesh.subdivide
    and subdivide_loop, open3d's subdivide_midpoint and subdivide_loop on the CPU) -> Subdivided.  A level splits every
    edge with two different ends (the rows of the EdgeTable, in its order: the new vertices follow the old ones in edge
    order) and every face into four, (v0, m0, m2), (m0, v1, m1), (m2, m1, v2), (m0, m1, m2) with m_k on the edge from
    corner k to the next: V + E vertices, 4 F faces, the parent's winding.  A face with a repeated vertex goes through the
    templates of subdivide_to_edge and stays degenerate.
    scheme="midpoint": a new vertex is (p_u + p_v) 0.5 and the old ones stay; the surface does not change.
    scheme="loop": Loop's scheme with Warren's weights.  A new vertex on an edge with exactly two faces is
    (p_u + p_v) 0.375 + (p_a + p_b) 0.125, a and b the opposite corners; on any other edge (a border, or three and more
    faces: a crease) the midpoint.  An old vertex on an edge with three or more faces, one whose number of border edges
    is neither 0 nor 2, and one without neighbours stay; one with two border edges moves to p 0.75 + (p_b0 + p_b1) 0.125;
    any other moves to p (1 - n beta) + s beta with s the sum of its n neighbours in ascending index and beta = 3 / 16
    for n = 3, else 3 / (8 n).  trimesh's subdivide_loop knows borders but no creases.
    `attributes` [V, k] go through the weights of the positions column by column.  float64 inside, cast at the end;
    no atomics, identical from run to run.  An empty mesh and levels = 0 return the input."""
    levels = _count(levels, "levels")
    if scheme not in _SUBDIVIDE_SCHEMES:
        raise ValueError(f"scheme must be 'loop' or 'midpoint' (got {scheme!r})")
    return _subdivide(verts, faces, attributes, _SUBDIVIDE_SCHEMES[scheme], None, levels, _info)


def subdivide_to_edge(verts, faces, max_edge, max_rounds=32, attributes=None, _info=None):
    """splits edges at their midpoints until none is longer than `max_edge` -> Subdivided.  A round marks the edges with
    (dx dx + dy dy) + dz dz > max_edge max_edge in float64 (a NaN length is not marked), gives each a new vertex at its
    midpoint and replaces every face by the template of its marked half-edges, in the parent's winding: none, the face;
    one, on the half-edge a -> b opposite c: (a, m, c), (m, b, c); two, a -> b unmarked: (m1, c, m2) and the quad
    a b m1 m2 along the shorter of its diagonals a-m1 and b-m2 (on a tie a-m1 exactly when a < b): (a, b, m1),
    (a, m1, m2) or (a, b, m2), (b, m1, m2); three: the four faces of subdivide_mesh.  Marks are per edge, so the faces on
    both sides split it and the mesh stays conforming; the surface does not change.  The rounds end when one marks
    nothing or after `max_rounds` of them: then `converged` is False and `longest_edge` says where the mesh stands.  After
    k rounds the longest edge is at most max_edge + (L - max_edge) / 2^k for an input whose longest is L (a diagonal of
    the two-marked template is a median, at most half the sum of two sides).  trimesh's subdivide_to_size splits every
    face in four until all edges are short.  One read-back per round; identical from run to run."""
    max_edge = _finite(max_edge, "max_edge", positive=True)
    max_rounds = _count(max_rounds, "max_rounds")
    return _subdivide(verts, faces, attributes, 0, max_edge, max_rounds, _info)


class Remeshed(NamedTuple):
    """verts [V', 3] in the input's dtype; faces [F', 3] int64; attributes [V', k] in their input's dtype, or None;
    iterations: the iterations run; collapsed / flipped / split: per iteration the edges collapsed, flipped and split"""
    verts: torch.Tensor
    faces: torch.Tensor
    attributes: torch.Tensor | None
    iterations: int
    collapsed: tuple
    flipped: tuple
    split: tuple


REMESH_STATUS_NAMES = {v: k.lower() for k, v in _lib.REMESH.items()}
_REMESH_RING_PASSES = 2      # passes over the one-rings after the pass over the edges: two winning collapses then share no
                             # vertex of the closed neighbourhoods of their ends (include/nudf.h, collapse_apply)


class _RemeshTables(NamedTuple):
    """what one sub-round reads besides the mesh; the descriptor keeps pointers into all of it: the caller holds it"""
    d: _lib.MeshTopo
    table: EdgeTable
    vclass: torch.Tensor
    ring_off: torch.Tensor
    held: tuple


def _remesh_tables(pos, faces):
    """the edge table, one-rings, border CSR, vertex classes, corner lists and the CSR of the edges at each vertex (both
    ends of the table's rows under one stable sort) of a mesh, and a descriptor that points at them"""
    n_verts, dev = pos.shape[0], pos.device
    table = _mesh_edges(faces, n_verts)
    n_edges = table.edges.shape[0]
    ring_off, ring = _vertex_adjacency(faces, n_verts, table)
    boundary = _boundary(table, n_verts)
    vclass = _loop_classes(table, boundary, n_verts)
    corner_off, corner = _corner_lists(faces, n_verts)
    ends = torch.cat([table.edges[:, 0], table.edges[:, 1]])
    vedge = (torch.sort(ends, stable=True).indices % max(n_edges, 1)).contiguous()
    vedge_off = torch.zeros(n_verts + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(ends, minlength=n_verts), 0, out=vedge_off[1:])
    d = _topo(faces, n_verts, table)
    d.pos = ptr(pos)
    d.sp_sd_ring_off, d.sp_sd_ring, d.sp_sd_n_ring = ptr(ring_off), ptr(ring), ring.numel()
    d.nbr_off, d.nbr, d.sp_sd_n_border = ptr(boundary.nbr_off), ptr(boundary.nbr), boundary.nbr.numel()
    d.sp_sd_vclass = ptr(vclass)
    d.sp_sd_hf_rm_corner_off, d.sp_sd_hf_rm_corner = ptr(corner_off), ptr(corner)
    d.sp_sd_hf_rm_vedge_off, d.sp_sd_hf_rm_vedge, d.sp_sd_hf_rm_n_vedge = ptr(vedge_off), ptr(vedge), vedge.numel()
    return _RemeshTables(d, table, vclass, ring_off, (pos, faces, ring, boundary, corner_off, corner, vedge_off, vedge))


def _remesh_ranks(status, key):
    """-> [E] the place of each candidate (status 0) in a stable sort by `key`, ties by edge index; E for the others"""
    n_edges = status.numel()
    cand = torch.nonzero(status == 0).reshape(-1)
    rank = torch.full((n_edges,), n_edges, dtype=torch.int64, device=status.device)
    rank[cand[torch.sort(key[cand], stable=True).indices]] = torch.arange(cand.numel(), dtype=torch.int64, device=status.device)
    return rank


def _remesh_best(t, status, rank, passes):
    """the minimum passes of one sub-round -> best [V]; `passes`: (mode, ...) in order"""
    d, dev = t.d, status.device
    n_verts = t.vclass.numel()
    d.sp_sd_hf_rm_status, d.sp_sd_hf_rm_rank = ptr(status), ptr(rank)
    best = None
    for mode in passes:
        out = torch.empty(n_verts, dtype=torch.int64, device=dev)
        d.sp_sd_hf_rm_mode, d.sp_sd_hf_rm_best_in, d.sp_sd_hf_rm_best_out = mode, ptr(best), ptr(out)
        call("nudf_meshremesh_vertex_min", d)
        best = out
    d.sp_sd_hf_rm_best_in = ptr(best)
    return best


def _repeats(faces):
    """-> [F] bool: two corners of the face are the same vertex"""
    return (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])


def _collapse_round(pos, faces, low, high, cos_border, counts=None):
    """one sub-round of collapses -> (winners, pos', faces'); the vertices that went stay in pos' unused"""
    t = _remesh_tables(pos, faces)
    d, dev = t.d, pos.device
    n_edges = t.table.edges.shape[0]
    status = torch.empty(n_edges, dtype=torch.uint8, device=dev)
    keep = torch.empty(n_edges, dtype=torch.int64, device=dev)
    gone = torch.empty(n_edges, dtype=torch.int64, device=dev)
    d.sp_sd_hf_rm_status, d.sp_sd_hf_rm_keep, d.sp_sd_hf_rm_gone = ptr(status), ptr(keep), ptr(gone)
    d.sp_sd_hf_rm_low, d.sp_sd_hf_rm_high, d.sp_sd_hf_rm_cos_border = low, high, cos_border
    call("nudf_meshremesh_collapse_check", d)
    n_cand = int((status == 0).sum())
    n_win = 0
    if n_cand:
        e = t.table.edges
        diff = pos[e[:, 0]] - pos[e[:, 1]]
        d2 = diff * diff
        rank = _remesh_ranks(status, (d2[:, 0] + d2[:, 1]) + d2[:, 2])
        best = _remesh_best(t, status, rank, (0,) + (1,) * _REMESH_RING_PASSES)
        remap = torch.arange(pos.shape[0], dtype=torch.int64, device=dev)
        pos_out = pos.clone()
        win = torch.empty(n_edges, dtype=torch.uint8, device=dev)
        d.sp_sd_hf_rm_remap, d.sp_sd_hf_rm_pos_out, d.sp_sd_hf_rm_win = ptr(remap), ptr(pos_out), ptr(win)
        call("nudf_meshremesh_collapse_apply", d)
        n_win = int(win.sum())
        if n_win:
            mapped = remap[faces]                       # a face that came with a repeated vertex stays
            pos, faces = pos_out, mapped[~_repeats(mapped) | _repeats(faces)].contiguous()
    if counts is not None:
        counts.append(dict(candidates=n_cand, winners=n_win))
    return n_win, pos, faces


def _flip_round(pos, faces, counts=None):
    """one sub-round of flips -> (winners, faces')"""
    t = _remesh_tables(pos, faces)
    d, dev = t.d, pos.device
    n_edges = t.table.edges.shape[0]
    status = torch.empty(n_edges, dtype=torch.uint8, device=dev)
    gain = torch.empty(n_edges, dtype=torch.int32, device=dev)
    ab = torch.empty((n_edges, 2), dtype=torch.int64, device=dev)
    d.sp_sd_hf_rm_status, d.sp_sd_hf_rm_gain, d.sp_sd_hf_rm_ab = ptr(status), ptr(gain), ptr(ab)
    call("nudf_meshremesh_flip_check", d)
    n_cand = int((status == 0).sum())
    n_win = 0
    if n_cand:
        rank = _remesh_ranks(status, -gain.to(torch.int64))
        best = _remesh_best(t, status, rank, (2,))
        out = faces.clone()
        win = torch.empty(n_edges, dtype=torch.uint8, device=dev)
        d.sp_sd_hf_rm_faces_out, d.sp_sd_hf_rm_win = ptr(out), ptr(win)
        call("nudf_meshremesh_flip_apply", d)
        n_win = int(win.sum())
        if n_win:
            faces = out
        del best
    if counts is not None:
        counts.append(dict(candidates=n_cand, winners=n_win))
    return n_win, faces


def _relax(pos, faces):
    """-> (pos', moving [V] bool: the smooth vertices with a one-ring, which relax moves)"""
    t = _remesh_tables(pos, faces)
    out = torch.empty_like(pos)
    t.d.sp_sd_hf_rm_pos_out = ptr(out)
    call("nudf_meshremesh_relax", t.d)
    return out, (t.vclass == 0) & (t.ring_off[1:] > t.ring_off[:-1])


def remesh_isotropic(verts, faces, target_edge, iterations=5, project=True, border_angle=30.0, attributes=None,
                     max_subrounds=16, _info=None):
    """isotropic remeshing towards edges of length `target_edge` (csrc/meshremesh.hip; pymeshlab, CGAL or trimesh.remesh on
    the CPU) -> Remeshed: the loop of Botsch and Kobbelt, "A remeshing approach to multiresolution modeling" (2004).
    With low = 0.8 target_edge and high = 4/3 target_edge an iteration
      1. splits the edges longer than high (subdivide_to_edge);
      2. collapses edges shorter than low in sub-rounds, until one has no winner or after `max_subrounds`, then drops the
         vertices that went (compact_mesh).  An edge with two faces between two smooth vertices goes to its midpoint; a
         border vertex is kept where it is; an edge between two border vertices that is not a border edge stays; a
         border edge is collapsed only where the border turns by less than `border_angle` degrees at the end that goes
         (0: the border keeps all its vertices).  No collapse changes the topology (link condition), makes an edge longer
         than high, turns a face over or merges two faces; vertices on an edge with three or more faces, those whose
         border is not a simple curve (_loop_classes' class 2) and the faces at them are left alone;
      3. flips edges with two faces in sub-rounds, stopped the same way, where that brings the valences of the four
         vertices nearer 6 (4 on the border) without a fold and the new edge does not exist;
      4. moves every smooth vertex to the mean of its one-ring, taken back into its tangent plane, and with `project`
         then to its closest point on the input mesh (one evaluation.MeshIndex, built once).  Border vertices stay.
    A sub-round takes an independent set of the candidates: each gets a rank (collapses: shorter first; flips: larger
    gain first; ties by edge index) and wins when it holds the smallest rank of its neighbourhood, found by per-vertex
    minimum passes -- no atomics, identical from run to run, and nothing depends on the winding or the order of the faces.
    `attributes` [V, k] are carried at the end from the input by transfer_attributes.  float64 inside, cast at the end.
    Not done: feature or crease preservation (a cube's edges are rounded), adaptive sizing, area-weighted relaxation.
    (`_info`: receives per iteration the sub-rounds' candidate and winner counts and, with an "events" dict in it, a pair
    of events per stage.)"""
    target_edge = _finite(target_edge, "target_edge", positive=True)
    iterations = _count(iterations, "iterations")
    max_subrounds = _count(max_subrounds, "max_subrounds")
    border_angle = _finite(border_angle, "border_angle")
    if not 0.0 <= border_angle <= 180.0:
        raise ValueError(f"border_angle must be in [0, 180] degrees (got {border_angle!r})")
    verts, faces = _check_mesh(verts, faces)
    attributes = _check_attributes(attributes, verts)
    if verts.shape[0] == 0 or faces.shape[0] == 0 or iterations == 0:
        return Remeshed(verts, faces, attributes, iterations, (0,) * iterations, (0,) * iterations, (0,) * iterations)
    low, high = 0.8 * target_edge, target_edge * 4 / 3
    cos_border = math.cos(math.radians(border_angle))
    events = None if _info is None else _info.get("events")
    pos, out_faces = verts.double().contiguous(), faces
    index = None
    if project:
        from . import evaluation
        index = evaluation.MeshIndex(pos, faces)
    collapsed, flipped, split, rounds = [], [], [], []
    for it in range(iterations):
        stages = None if events is None else events.setdefault(f"iteration{it}", {})
        state, log = {}, dict(collapse=[], flip=[])
        rounds.append(log)
        if out_faces.shape[0] == 0:
            collapsed.append(0), flipped.append(0), split.append(0)
            continue
        _stage(stages, state, "split")
        s = subdivide_to_edge(pos, out_faces, high)
        split.append(s.verts.shape[0] - pos.shape[0])
        pos, out_faces = s.verts, s.faces
        _stage(stages, state, "collapse")
        total = 0
        for _ in range(max_subrounds):
            n, pos, out_faces = _collapse_round(pos, out_faces, low, high, cos_border, log["collapse"])
            if n == 0:
                break
            total += n
        collapsed.append(total)
        pos, out_faces = compact_mesh(pos, out_faces)
        pos, out_faces = pos.contiguous(), out_faces.contiguous()
        _stage(stages, state, "flip")
        total = 0
        for _ in range(max_subrounds):
            if out_faces.shape[0] == 0:
                break
            n, out_faces = _flip_round(pos, out_faces, log["flip"])
            if n == 0:
                break
            total += n
        flipped.append(total)
        if out_faces.shape[0]:
            _stage(stages, state, "relax")
            new, moving = _relax(pos, out_faces)
            if index is not None:
                _stage(stages, state, "project")
                rows = torch.nonzero(moving).reshape(-1)
                if rows.numel():
                    c = index.closest(new[rows])
                    hit = c.face >= 0
                    new[rows[hit]] = c.point[hit]
            pos = new
        _stage(stages, state, None)
    attr = None
    if attributes is not None:
        attr = transfer_attributes(verts, faces, attributes, pos)
    if _info is not None:
        _info["rounds"] = rounds
    return Remeshed(pos.to(verts.dtype), out_faces, attr, iterations, tuple(collapsed), tuple(flipped), tuple(split))

def ellipse_footprint(ksize):
    """OpenCV's MORPH_ELLIPSE structuring element of size ksize x ksize -> np.uint8 [ksize, ksize], restated from the
    formula in its documentation: with r = c = ksize // 2, row i sets the columns [max(c - dx, 0), min(c + dx + 1, ksize))
    where dx = rint(c sqrt((r^2 - (i - r)^2) / r^2)).  It reproduces the 5 x 5 element printed there; cv2 itself is not
    available to check other sizes against."""
    ksize = int(ksize)
    if ksize < 1:
        raise ValueError(f"ksize must be >= 1 (got {ksize})")
    out = np.zeros((ksize, ksize), dtype=np.uint8)
    r = c = ksize // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    for i in range(ksize):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))
            out[i, max(c - dx, 0):min(c + dx + 1, ksize)] = 1
    return out


def dilate_masks(masks, ksize, chunk=8):
    """binary dilation of masks [n, H, W] (non-zero = set) with ellipse_footprint(ksize), anchored at its centre, pixels
    beyond the image unset (cv2.dilate's defaults) -> uint8 0 / 1 of the same shape and device.  Every footprint row is
    one run of columns: a horizontal running count per distinct run, OR-ed over the rows it occurs in."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3:
        raise ValueError("masks must be a [n, H, W] tensor")
    fp = ellipse_footprint(ksize)
    c = fp.shape[0] // 2
    runs = {}
    for i, row in enumerate(fp):
        cols = np.nonzero(row)[0]
        if len(cols):
            runs.setdefault((int(cols[0]) - c, int(cols[-1]) - c), []).append(i - c)
    n, H, W = masks.shape
    out = torch.zeros((n, H, W), dtype=torch.uint8, device=masks.device)
    xs = torch.arange(W, device=masks.device)
    for s in range(0, n, chunk):
        m = masks[s:s + chunk] != 0
        acc = torch.zeros_like(m)
        csum = torch.zeros((m.shape[0], H, W + 1), dtype=torch.int32, device=masks.device)
        torch.cumsum(m, 2, dtype=torch.int32, out=csum[:, :, 1:])
        for (lo, hi), dys in runs.items():
            # out(y, x) takes src(y + dy, x + dx) for dx in [lo, hi]
            a, b = (xs + lo).clamp(0, W), (xs + hi + 1).clamp(0, W)
            row_any = csum[:, :, b] > csum[:, :, a]
            for dy in dys:
                y0, y1 = max(0, -dy), min(H, H - dy)
                if y0 < y1:
                    acc[:, y0:y1] |= row_any[:, y0 + dy:y1 + dy]
        out[s:s + chunk] = acc
    return out


def load_dtu_views(dataset_dir, scan):
    """the cameras and object masks of a DTU scan as the reference's cleaning reads them (clean_dtu_mesh.py:37-52):
    <dataset_dir>/scan<scan>/cameras.npz (world_mat_<i>) and mask/*.png in sorted order, channel 0
    -> (world_mats np.float64 [n, 4, 4], masks np.uint8 [n, H, W], undilated: the object is where a mask is > 128)."""
    from PIL import Image
    root = os.path.join(str(dataset_dir), f"scan{scan}")
    files = sorted(glob.glob(os.path.join(root, "mask", "*.png")))
    if not files:
        raise FileNotFoundError(f"no mask/*.png under {root}")
    cams = np.load(os.path.join(root, "cameras.npz"))
    mats = np.stack([np.asarray(cams[f"world_mat_{i}"], dtype=np.float64) for i in range(len(files))])
    masks = []
    for f in files:
        m = np.asarray(Image.open(f))
        masks.append(np.ascontiguousarray(m[..., 0] if m.ndim == 3 else m).astype(np.uint8))
    return mats, np.stack(masks)


def view_counts(verts, world_mats, masks, border=0):
    """[V] int32: for each vertex the number of views in which it projects into a set mask pixel.  Per view
    q = P[:3, :3] p + P[:3, 3] in float64, each row as ((P0 x + P1 y) + P2 z) + P3; (x, y) = round-half-even(q.xy / q.z)
    + 1; the view counts when border <= x <= W - border, border <= y <= H - border and the mask, padded by one pixel of
    ones, is set at (y, x).  A non-finite q.xy / q.z counts for nothing.  There is no depth test, as in the reference."""
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise ValueError("verts must be a tensor on a GPU")
    if verts.dtype not in (torch.float32, torch.float64) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be float32 or float64 [V, 3] (got {verts.dtype} {tuple(verts.shape)})")
    dev = verts.device
    if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.dim() != 3:
        raise ValueError("masks must be a uint8 [n_views, H, W] tensor")
    if masks.device != dev:
        raise ValueError(f"masks must be on the vertices' GPU (got {masks.device})")
    mats = torch.as_tensor(np.asarray(world_mats.cpu() if isinstance(world_mats, torch.Tensor) else world_mats,
                                      dtype=np.float64))
    n, H, W = masks.shape
    if mats.dim() != 3 or mats.shape[0] != n or mats.shape[1] < 3 or mats.shape[2] != 4:
        raise ValueError(f"world_mats must be [{n}, 4, 4] like the masks (got {tuple(mats.shape)})")
    border = int(border)
    if border < 0 or H < 1 or W < 1:
        raise ValueError("border must be >= 0 and the masks not empty")
    proj = mats[:, :3, :].contiguous().to(dev)
    pos = verts.double().contiguous()
    masks = masks.contiguous()
    count = torch.zeros(verts.shape[0], dtype=torch.int32, device=dev)
    d = _lib.MeshTopo(pos=ptr(pos), proj=ptr(proj), masks=ptr(masks), vis_count=ptr(count), n_verts=verts.shape[0],
                      n_views=n, H=H, W=W, border=border)
    call("nudf_meshtopo_views", d)
    return count


def clean_by_views(verts, faces, world_mats, masks, mode="mask", minimal_vis=0, max_outside=HULL_MAX_OUTSIDE,
                   border=HULL_BORDER, drop_unreferenced=False):
    """cuts the mesh by what the views see (clean_dtu_mesh.py:36-154) -> (verts', faces').
    mode "mask": masks [n, H, W] uint8 are the (dilated) object masks; a vertex stays when more than minimal_vis views
    see it inside one (window 0 <= x <= W, 0 <= y <= H after the reference's shift by one).
    mode "hull": the masks are set *outside* the dilated object; the window shrinks by `border` on each side and a vertex
    stays when fewer than max_outside views see it outside (the reference hard-codes 5 and ignores minimal_vis here).
    Faces with a dropped vertex go.  Vertices that pass stay even when no face uses them any more, as in the reference
    (the DTU evaluation samples every vertex); drop_unreferenced=True removes them."""
    if mode not in ("mask", "hull"):
        raise ValueError(f"mode must be 'mask' or 'hull' (got {mode!r})")
    verts, faces = _check_mesh(verts, faces)
    if verts.shape[0] == 0:
        return verts, faces
    count = view_counts(verts, world_mats, masks, border if mode == "hull" else 0)
    keep = count > int(minimal_vis) if mode == "mask" else count < int(max_outside)
    return compact_mesh(verts, faces, vertex_mask=keep, drop_unreferenced=drop_unreferenced)


def clean_dtu_mesh(verts, faces, world_mats, masks, mask_dilated_size=11, minimal_vis=2):
    """the reference's DTU cleaning sequence (clean_dtu_mesh.py __main__): mask cleaning with the object masks (> 128)
    dilated by mask_dilated_size, then visual-hull cleaning against the masks dilated by mask_dilated_size + 20 (outside =
    dilated value < 128).  masks: the undilated uint8 [n, H, W] masks of load_dtu_views -> (verts', faces')"""
    verts, faces = _check_mesh(verts, faces)
    if not isinstance(masks, torch.Tensor):
        masks = torch.as_tensor(np.asarray(masks))
    masks = masks.to(verts.device)
    inside = dilate_masks(masks > 128, mask_dilated_size)
    verts, faces = clean_by_views(verts, faces, world_mats, inside, "mask", minimal_vis=minimal_vis)
    del inside
    outside = 1 - dilate_masks(masks >= 128, mask_dilated_size + 20)
    return clean_by_views(verts, faces, world_mats, outside, "hull")
