"""numpy float64 restatement of csrc/meshsubdiv.hip and of meshclean.subdivide_mesh / subdivide_to_edge, operation by
operation (include/nudf.h states the definitions).  numpy does not contract a product into a sum.  Elementwise expressions
are written once for all items; the one sum of varying length, the one-ring of Loop's vertex rule, is a plain loop per
vertex, in list order from the first neighbour.  The face templates involve floats only in the choice of a diagonal.
Faces are taken to be in range: the host checks them."""
import math
from typing import NamedTuple

import numpy as np

import meshray_ref
import meshsmooth_ref

SCHEMES = ("midpoint", "loop")


# ---- the edge table (meshclean.EdgeTable) ---------------------------------------------------------------------------------
class Edges(NamedTuple):
    u: np.ndarray            # [E] the smaller end
    v: np.ndarray            # [E] the larger end; rows ordered by (u, v)
    count: np.ndarray        # [E] half-edges on the edge
    he_edge: np.ndarray      # [3 F] the edge of half-edge 3 f + k (faces[f][k] -> faces[f][(k + 1) % 3])
    he_id: np.ndarray        # [3 F] the half-edges ordered by edge, ascending inside each
    edge_start: np.ndarray   # [E] the first position of each edge in he_id


def edge_table(faces, n_verts):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, 1).reshape(-1)
    key = np.minimum(a, b) * max(n_verts, 1) + np.maximum(a, b)
    he_id = np.argsort(key, kind="stable").astype(np.int64)
    skey = key[he_id]
    first = np.ones(len(skey), bool)
    first[1:] = skey[1:] != skey[:-1]
    edge_start = np.nonzero(first)[0].astype(np.int64)
    he_edge = np.empty(len(key), np.int64)
    he_edge[he_id] = np.cumsum(first) - 1
    ekey = skey[edge_start]
    count = np.diff(np.append(edge_start, len(skey))).astype(np.int64)
    return Edges(ekey // max(n_verts, 1), ekey % max(n_verts, 1), count, he_edge, he_id, edge_start)


def _dist2(p, q):
    d = p - q
    d2 = d * d
    return (d2[..., 0] + d2[..., 1]) + d2[..., 2]


def longest_edge(pos, table):
    keep = table.u != table.v
    if not keep.any():
        return 0.0
    return math.sqrt(float(_dist2(pos[table.u[keep]], pos[table.v[keep]]).max()))


# ---- mark -----------------------------------------------------------------------------------------------------------------
def mark(pos, table, max_edge=None):
    """[E] bool: the edge is split.  max_edge None: every edge with two different ends"""
    proper = table.u != table.v
    if max_edge is None:
        return proper
    with np.errstate(invalid="ignore"):
        return proper & (_dist2(pos[table.u], pos[table.v]) > max_edge * max_edge)     # NaN > x is False


def edge_vertices(marks, n_verts):
    """[E] the new vertex of each marked edge, n_verts + its rank among them, -1 for the others"""
    return np.where(marks, n_verts + np.cumsum(marks) - 1, -1).astype(np.int64)


# ---- odd: the new vertices --------------------------------------------------------------------------------------------------
def odd(x, faces, table, marks, scheme):
    """rows for the marked edges, in edge order, of any per-vertex columns x [V, k] (positions, attributes)"""
    e = np.nonzero(marks)[0]
    xu, xv = x[table.u[e]], x[table.v[e]]
    out = (xu + xv) * 0.5
    if scheme == "loop":
        two = table.count[e] == 2
        s = table.edge_start[e[two]]
        h0, h1 = table.he_id[s], table.he_id[s + 1]
        assert (h0 < h1).all()
        a, b = faces[h0 // 3, (h0 % 3 + 2) % 3], faces[h1 // 3, (h1 % 3 + 2) % 3]
        out[two] = (xu[two] + xv[two]) * 0.375 + (x[a] + x[b]) * 0.125
    return out


# ---- even: the old vertices -------------------------------------------------------------------------------------------------
def border_lists(table, n_verts):
    """the other ends of the edges with one half-edge at each vertex, ascending (both directions of every such edge)"""
    out = [[] for _ in range(n_verts)]
    for u, v, c in zip(table.u.tolist(), table.v.tolist(), table.count.tolist()):
        if c == 1:
            out[u].append(v)
            out[v].append(u)
    return [sorted(r) for r in out]


def vertex_classes(table, n_verts, border=None):
    """[V] 0 smooth, 1 border (two border edges), 2 stays (on an edge with three or more half-edges, or a number of border
    edges other than 0 and 2)"""
    border = border_lists(table, n_verts) if border is None else border
    deg = np.array([len(r) for r in border], np.int64).reshape(-1)
    cls = np.zeros(n_verts, np.uint8)
    cls[deg == 2] = 1
    cls[(deg != 0) & (deg != 2)] = 2
    multi = table.count >= 3
    cls[table.u[multi]] = 2
    cls[table.v[multi]] = 2
    return cls


def even(x, faces, table, scheme):
    """rows for the old vertices of any per-vertex columns x [V, k]"""
    out = x.copy()
    if scheme != "loop":
        return out
    n_verts = len(x)
    border = border_lists(table, n_verts)
    cls = vertex_classes(table, n_verts, border)
    off, ring = meshsmooth_ref.vertex_adjacency(faces, n_verts)
    for v in range(n_verts):
        if cls[v] == 1:
            b0, b1 = border[v]
            out[v] = x[v] * 0.75 + (x[b0] + x[b1]) * 0.125
        elif cls[v] == 0 and off[v + 1] > off[v]:
            r = ring[off[v]:off[v + 1]]
            n = len(r)
            s = x[r[0]].copy()
            for w in r[1:]:
                s = s + x[w]
            nd = float(n)
            beta = 0.1875 if n == 3 else 3.0 / (8.0 * nd)
            out[v] = x[v] * (1.0 - nd * beta) + s * beta
    return out


# ---- count and emit: the faces -------------------------------------------------------------------------------------------------
def face_marks(table, edge_vertex, n_faces):
    """[F, 3] the new vertex of each half-edge or -1"""
    return edge_vertex[table.he_edge].reshape(n_faces, 3)


def count(table, edge_vertex, n_faces):
    return 1 + (face_marks(table, edge_vertex, n_faces) >= 0).sum(1).astype(np.int64)


def emit(faces, table, edge_vertex, pos_out):
    """-> (faces' [F', 3], parent [F']) by the four templates; pos_out decides the diagonal of the two-marked one"""
    n_faces = len(faces)
    m = face_marks(table, edge_vertex, n_faces)
    n = (m >= 0).sum(1)
    cnt = n + 1
    off = np.cumsum(cnt) - cnt
    out = np.full((int(cnt.sum()), 3), -1, np.int64)
    parent = np.repeat(np.arange(n_faces, dtype=np.int64), cnt)
    rows = np.arange(n_faces)

    def corners(i, k):
        return faces[i, k], faces[i, (k + 1) % 3], faces[i, (k + 2) % 3]

    i = rows[n == 0]
    out[off[i]] = faces[i]
    i = rows[n == 1]
    k = np.argmax(m[i] >= 0, 1)
    a, b, c = corners(i, k)
    mk = m[i, k]
    out[off[i]] = np.stack([a, mk, c], 1)
    out[off[i] + 1] = np.stack([mk, b, c], 1)
    i = rows[n == 2]
    k = np.argmax(m[i] < 0, 1)
    a, b, c = corners(i, k)
    m1, m2 = m[i, (k + 1) % 3], m[i, (k + 2) % 3]
    out[off[i]] = np.stack([m1, c, m2], 1)
    with np.errstate(invalid="ignore"):
        da, db = _dist2(pos_out[a], pos_out[m1]), _dist2(pos_out[b], pos_out[m2])
        along_a = (da < db) | (~(da > db) & (a < b))
    out[off[i] + 1] = np.where(along_a[:, None], np.stack([a, b, m1], 1), np.stack([a, b, m2], 1))
    out[off[i] + 2] = np.where(along_a[:, None], np.stack([a, m1, m2], 1), np.stack([b, m1, m2], 1))
    i = rows[n == 3]
    v0, v1, v2 = faces[i, 0], faces[i, 1], faces[i, 2]
    m0, m1, m2 = m[i, 0], m[i, 1], m[i, 2]
    out[off[i]] = np.stack([v0, m0, m2], 1)
    out[off[i] + 1] = np.stack([m0, v1, m1], 1)
    out[off[i] + 2] = np.stack([m2, m1, v2], 1)
    out[off[i] + 3] = np.stack([m0, m1, m2], 1)
    return out, parent


# ---- the drivers ----------------------------------------------------------------------------------------------------------
class Subdivided(NamedTuple):
    verts: np.ndarray
    faces: np.ndarray
    attributes: np.ndarray
    parent_face: np.ndarray
    rounds: int
    longest_edge: float
    converged: bool


def one_round(pos, faces, attr, scheme, max_edge=None, marks=None):
    """-> (edges marked, pos', faces', attr', parent); faces' None when nothing is marked.  `marks`: given ones, for the
    template tests"""
    table = edge_table(faces, len(pos))
    marks = mark(pos, table, max_edge) if marks is None else np.asarray(marks, bool)
    if not marks.any():
        return 0, pos, None, attr, None
    pos_out = np.concatenate([even(pos, faces, table, scheme), odd(pos, faces, table, marks, scheme)])
    attr_out = None if attr is None else np.concatenate([even(attr, faces, table, scheme),
                                                         odd(attr, faces, table, marks, scheme)])
    faces_out, parent = emit(faces, table, edge_vertices(marks, len(pos)), pos_out)
    return int(marks.sum()), pos_out, faces_out, attr_out, parent


def _drive(verts, faces, attributes, scheme, max_edge, cap):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = np.arange(len(faces), dtype=np.int64)
    if len(verts) == 0 or len(faces) == 0:
        return Subdivided(verts, faces, attributes, parent, 0, 0.0, True)
    pos = np.asarray(verts, np.float64)
    attr = None if attributes is None else np.asarray(attributes, np.float64)
    rounds, converged = 0, True
    while max_edge is not None or rounds < cap:
        if rounds == cap:
            converged = not mark(pos, edge_table(faces, len(pos)), max_edge).any()
            break
        n_marked, pos, new_faces, attr, new_parent = one_round(pos, faces, attr, scheme, max_edge)
        if new_faces is None:
            break
        faces, parent, rounds = new_faces, parent[new_parent], rounds + 1
    return Subdivided(pos.astype(verts.dtype), faces, None if attributes is None else attr.astype(attributes.dtype), parent,
                      rounds, longest_edge(pos, edge_table(faces, len(pos))), converged)


def subdivide_mesh(verts, faces, levels=1, scheme="loop", attributes=None):
    return _drive(verts, faces, attributes, scheme, None, levels)


def subdivide_to_edge(verts, faces, max_edge, max_rounds=32, attributes=None):
    return _drive(verts, faces, attributes, "midpoint", float(max_edge), max_rounds)


# ---- the test meshes and their measures -------------------------------------------------------------------------------------
def stretched_sheet():
    """meshray_ref.grid_sheet(4) stretched 50 : 1 along x"""
    v, f = meshray_ref.grid_sheet(4)
    v = np.array(v, np.float64)
    v[:, 0] *= 50.0
    return v, f


def meshes():
    """the eight meshes of the issue, name -> (verts, faces)"""
    out = dict(sphere=meshsmooth_ref.noisy_sphere(), cube=meshsmooth_ref.noisy_cube()[:2],
               sheet=meshsmooth_ref.noisy_sheet()[:2], fan=meshsmooth_ref.fan_mesh(), three=meshsmooth_ref.three_on_an_edge(),
               awkward=meshsmooth_ref.awkward_mesh(), ico0=meshray_ref.icosphere(0), stretched=stretched_sheet())
    return {k: (np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)) for k, (v, f) in out.items()}


def face_normals(pos, faces):
    """(p1 - p0) x (p2 - p0), not normalised: its length is twice the area"""
    p0, p1, p2 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    return np.cross(p1 - p0, p2 - p0)


def area(pos, faces):
    return float(0.5 * np.linalg.norm(face_normals(pos, faces), axis=1).sum())


def euler(pos, faces):
    """(V used, E, F, histogram {half-edges on an edge: edges}) over the edges with two different ends"""
    t = edge_table(faces, len(pos))
    keep = t.u != t.v
    hist = {int(c): int(n) for c, n in zip(*np.unique(t.count[keep], return_counts=True))}
    return len(np.unique(faces)), int(keep.sum()), len(faces), hist


def expected_rounds(longest, max_edge):
    return max(0, math.ceil(math.log2(longest / max_edge)))
