"""numpy float64 restatement of csrc/meshremesh.hip and of meshclean.remesh_isotropic, operation by operation
(include/nudf.h states the definitions).  numpy does not contract a product into a sum; its square root and division are
correctly rounded.  The tests of an edge that are cheap are written once for all edges; the walks of the edges that pass
them (the merge of two one-rings, the faces at the ends, the edges at a vertex) are plain loops in the kernels' order.
The split is meshsubdiv_ref's, the projection meshdist_ref's.  Faces are taken to be in range: the host checks them."""
import math
from typing import NamedTuple

import numpy as np

import meshdist_ref
import meshray_ref
import meshsmooth_ref
import meshsubdiv_ref as S

(CANDIDATE, COUNT, LONG, CLASS, BORDER, LINK, REACH, FOLD, DUPLICATE, SAME, EXISTS, GAIN) = range(12)


# ---- the tables the driver builds between the launches ---------------------------------------------------------------------
class Topo(NamedTuple):
    table: S.Edges
    face0: np.ndarray        # [E] the face of the first half-edge of each edge
    face1: np.ndarray        # [E] that of the second, or -1
    edge_key: np.ndarray     # [E] u * V + v, ascending
    ring_off: np.ndarray
    ring: np.ndarray         # the one-rings, ascending
    border: list             # the border neighbours of each vertex, ascending
    vclass: np.ndarray       # [V] 0 smooth, 1 border, 2 stays
    corner_off: np.ndarray
    corner: np.ndarray       # the corners 3 f + k by vertex, ascending
    vedge_off: np.ndarray
    vedge: np.ndarray        # the rows of the edge table at each vertex: a stable sort of (all u, then all v)


def topo(faces, n_verts):
    t = S.edge_table(faces, n_verts)
    n_edges = len(t.u)
    face0 = t.he_id[t.edge_start] // 3 if n_edges else np.zeros(0, np.int64)
    face1 = np.full(n_edges, -1, np.int64)
    two = t.count >= 2
    face1[two] = t.he_id[t.edge_start[two] + 1] // 3
    ring_off, ring = meshsmooth_ref.vertex_adjacency(faces, n_verts)
    border = S.border_lists(t, n_verts)
    corner_off, corner = meshsmooth_ref.corners(faces, n_verts)
    ends = np.concatenate([t.u, t.v])
    vedge = (np.argsort(ends, kind="stable") % max(n_edges, 1)).astype(np.int64)
    vedge_off = np.zeros(n_verts + 1, np.int64)
    vedge_off[1:] = np.cumsum(np.bincount(ends, minlength=n_verts))
    return Topo(t, face0, face1, t.u * max(n_verts, 1) + t.v, ring_off, ring.astype(np.int64).reshape(-1), border,
                S.vertex_classes(t, n_verts, border), corner_off, corner, vedge_off, vedge)


def ring_of(T, w):
    return T.ring[T.ring_off[w]:T.ring_off[w + 1]]


def valence(T):
    return np.diff(T.ring_off)


def target_valence(T):
    return np.where(T.vclass == 1, 4, 6)


# ---- float64 helpers in the kernels' order --------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dist2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def normals(tri, pos):
    """tri [..., 3] vertex indices -> (p1 - p0) x (p2 - p0) with the corners rotated so that the smallest index (its first
    occurrence) comes first"""
    tri = np.asarray(tri, np.int64)
    k = np.argmin(tri, -1)[..., None]
    i0, i1, i2 = (np.take_along_axis(tri, (k + j) % 3, -1)[..., 0] for j in range(3))
    return _cross(pos[i1] - pos[i0], pos[i2] - pos[i0])


def _normals_moved(tri, pos, u, v, p):
    """the same with the ends u and v both at p"""
    k = np.argmin(tri, -1)[..., None]
    idx = np.take_along_axis(tri, (k + np.arange(3)) % 3, -1)
    q = pos[idx]
    q[(idx == u) | (idx == v)] = p
    return _cross(q[..., 1, :] - q[..., 0, :], q[..., 2, :] - q[..., 0, :])


def opposite(faces, h):
    return faces[h // 3, (h % 3 + 2) % 3]


# ---- collapse_check --------------------------------------------------------------------------------------------------------
def _common(T, u, v):
    a, b = ring_of(T, u), ring_of(T, v)
    i = j = n = 0
    while i < len(a) and j < len(b):
        if a[i] == b[j]:
            n, i, j = n + 1, i + 1, j + 1
        elif a[i] < b[j]:
            i += 1
        else:
            j += 1
    return n


def _border_ok(pos, T, g, k, apex, cos_border):
    nb = T.border[g]
    if len(nb) != 2 or k not in nb:
        return False
    o = nb[1] if nb[0] == k else nb[0]
    if o == k or o == g or o == apex or not cos_border < 1.0:
        return False
    a, b = pos[g] - pos[o], pos[k] - pos[g]
    with np.errstate(invalid="ignore"):
        return bool(_dot(a, b) > (cos_border * np.sqrt(_dot(a, a))) * np.sqrt(_dot(b, b)))


def _geometry(pos, faces, T, u, v, gone, p, ca, cb, high):
    """the walks of one edge, each written once for all its items (every item's arithmetic is its own)"""
    if (T.vclass[ring_of(T, gone)] > 1).any():
        return CLASS
    with np.errstate(invalid="ignore", over="ignore"):
        ring = np.concatenate([ring_of(T, u), ring_of(T, v)])
        ring = ring[(ring != u) & (ring != v)]
        if not (_dist2(pos[ring], p) <= high * high).all():
            return REACH
        c = np.concatenate([T.corner[T.corner_off[w]:T.corner_off[w + 1]] for w in (u, v)])
        side = np.arange(len(c)) >= T.corner_off[u + 1] - T.corner_off[u]
        t = faces[c // 3]
        rest = ~((t == u).any(1) & (t == v).any(1))                    # a face with both ends goes with the edge
        c, side, t = c[rest], side[rest], t[rest]
        if not (_dot(normals(t, pos), _normals_moved(t, pos, u, v, p)) > 0.0).all():
            return FOLD
        rows = np.arange(len(c))
        x, y = t[rows, (c + 1) % 3], t[rows, (c + 2) % 3]
        twin = (ca >= 0) & (((x == ca) & (y == cb)) | ((x == cb) & (y == ca)))
    return DUPLICATE if (twin & ~side).any() and (twin & side).any() else CANDIDATE


def collapse_check(pos, faces, T, low, high, cos_border):
    """-> (status [E] uint8, keep [E], gone [E])"""
    t = T.table
    n_edges = len(t.u)
    status = np.full(n_edges, CANDIDATE, np.uint8)
    keep, gone = np.full(n_edges, -1, np.int64), np.full(n_edges, -1, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        short = _dist2(pos[t.u], pos[t.v]) < low * low
    cu, cv = T.vclass[t.u], T.vclass[t.v]
    status[(cu > 1) | (cv > 1)] = CLASS
    status[~short] = LONG
    status[((t.count != 1) & (t.count != 2)) | (t.u == t.v)] = COUNT
    for e in np.nonzero(status == CANDIDATE)[0]:
        u, v, s = int(t.u[e]), int(t.v[e]), t.edge_start[e]
        ca = int(opposite(faces, t.he_id[s]))
        if t.count[e] == 2:
            cb = int(opposite(faces, t.he_id[s + 1]))
            if cu[e] == 1 and cv[e] == 1:
                status[e] = BORDER
            elif _common(T, u, v) != 2:
                status[e] = LINK
            else:
                k, g = (v, u) if cv[e] == 1 else (u, v)
                p = pos[u] if cu[e] == 1 else (pos[v] if cv[e] == 1 else (pos[u] + pos[v]) * 0.5)
                status[e] = _geometry(pos, faces, T, u, v, g, p, ca, cb, high)
                keep[e], gone[e] = k, g
        else:
            first, second = _border_ok(pos, T, v, u, ca, cos_border), _border_ok(pos, T, u, v, ca, cos_border)
            if not first and not second:
                status[e] = BORDER
            elif _common(T, u, v) != 1:
                status[e] = LINK
            else:
                st = _geometry(pos, faces, T, u, v, v, pos[u], -1, -1, high) if first else BORDER
                keep[e], gone[e] = u, v
                if st != CANDIDATE and second:
                    other = _geometry(pos, faces, T, u, v, u, pos[v], -1, -1, high)
                    if other == CANDIDATE or not first:
                        st = other
                    if other == CANDIDATE:
                        keep[e], gone[e] = v, u
                status[e] = st
    bad = status != CANDIDATE
    keep[bad] = gone[bad] = -1
    return status, keep, gone


# ---- ranks and the minimum passes ------------------------------------------------------------------------------------------
def ranks(status, key):
    """[E] the place of each candidate in a stable sort by `key` (then edge index); n_edges for the others"""
    n_edges = len(status)
    cand = np.nonzero(status == CANDIDATE)[0]
    out = np.full(n_edges, n_edges, np.int64)
    out[cand[np.argsort(key[cand], kind="stable")]] = np.arange(len(cand))
    return out


def edge_length2(pos, T):
    with np.errstate(invalid="ignore", over="ignore"):
        return _dist2(pos[T.table.u], pos[T.table.v])


def vertex_min(T, faces, status, rank, mode, best_in=None):
    """a minimum does not depend on its order: scattered with np.minimum.at over the lists the kernel walks"""
    n_verts, n_edges = len(T.vclass), len(status)
    r = np.where((status == CANDIDATE) & (rank >= 0) & (rank < n_edges), rank, n_edges)
    out = np.full(n_verts, n_edges, np.int64)
    if mode == 0:
        np.minimum.at(out, T.table.u, r)
        np.minimum.at(out, T.table.v, r)
    elif mode == 1:
        out = best_in.copy()
        np.minimum.at(out, np.repeat(np.arange(n_verts), np.diff(T.ring_off)), best_in[T.ring])
    else:
        per_face = r[T.table.he_edge.reshape(-1, 3)].min(1)
        np.minimum.at(out, faces.reshape(-1), np.repeat(per_face, 3))
    return out


# ---- collapse_apply --------------------------------------------------------------------------------------------------------
def collapse_apply(pos, T, status, rank, keep, gone, best):
    """-> (remap [V], pos_out [V, 3], win [E] uint8)"""
    t = T.table
    n_edges = len(t.u)
    remap, pos_out = np.arange(len(pos), dtype=np.int64), pos.copy()
    win = (status == CANDIDATE) & (rank < n_edges) & (rank == np.minimum(best[t.u], best[t.v]))
    for e in np.nonzero(win)[0]:
        u, v = t.u[e], t.v[e]
        remap[gone[e]] = keep[e]
        mid = t.count[e] == 2 and T.vclass[u] == 0 and T.vclass[v] == 0
        pos_out[keep[e]] = (pos[u] + pos[v]) * 0.5 if mid else pos[keep[e]]
    return remap, pos_out, win.astype(np.uint8)


def map_faces(faces, remap):
    """the faces through remap, those that the collapses gave two equal corners dropped (a face that came with a
    repeated vertex stays)"""
    def repeats(t):
        return (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    f = remap[faces]
    return f[~repeats(f) | repeats(faces)]


# ---- flip_check and flip_apply ---------------------------------------------------------------------------------------------
def _children(faces, T, e):
    """the two parents' rows and the children of flipping the edges e (all with two faces)"""
    t = T.table
    h0, h1 = t.he_id[t.edge_start[e]], t.he_id[t.edge_start[e] + 1]
    a, b = opposite(faces, h0), opposite(faces, h1)
    t0, t1 = faces[h0 // 3], faces[h1 // 3]
    c0 = np.where(t0 == t.v[e][:, None], b[:, None], t0)
    c1 = np.where(t1 == t.u[e][:, None], a[:, None], t1)
    alike = (faces.reshape(-1)[h0] == t.u[e]) != (faces.reshape(-1)[h1] == t.u[e])
    return h0 // 3, h1 // 3, a, b, t0, t1, c0, c1, alike


def flip_check(pos, faces, T):
    """-> (status [E] uint8, gain [E] int32, ab [E, 2])"""
    t = T.table
    n_edges, n_verts = len(t.u), len(pos)
    status = np.full(n_edges, COUNT, np.uint8)
    gain, ab = np.zeros(n_edges, np.int32), np.full((n_edges, 2), -1, np.int64)
    e = np.nonzero((t.count == 2) & (t.u != t.v))[0]
    if len(e) == 0:
        return status, gain, ab
    f0, f1, a, b, t0, t1, c0, c1, alike = _children(faces, T, e)
    u, v = t.u[e], t.v[e]
    same = (a == b) | (a == u) | (a == v) | (b == u) | (b == v) | (f0 == f1)
    cls = T.vclass
    klass = (cls[u] > 1) | (cls[v] > 1) | (cls[a] > 1) | (cls[b] > 1)
    exists = np.isin(np.minimum(a, b) * n_verts + np.maximum(a, b), T.edge_key)
    dev = valence(T) - target_valence(T)
    g = ((dev[u] ** 2 + dev[v] ** 2 + dev[a] ** 2 + dev[b] ** 2)
         - ((dev[u] - 1) ** 2 + (dev[v] - 1) ** 2 + (dev[a] + 1) ** 2 + (dev[b] + 1) ** 2))
    with np.errstate(invalid="ignore", over="ignore"):
        n0, n1, m0, m1 = normals(t0, pos), normals(t1, pos), normals(c0, pos), normals(c1, pos)
        c = np.where(alike, 1.0, -1.0)
        fine = (_dot(m0, n0) > 0.0) & (_dot(m1, n1) > 0.0) & (c * _dot(m0, n1) > 0.0) & (c * _dot(m1, n0) > 0.0)
    st = np.full(len(e), CANDIDATE, np.uint8)
    st[~fine] = FOLD
    st[~(g > 0)] = GAIN
    st[exists] = EXISTS
    st[klass] = CLASS
    st[same] = SAME
    status[e] = st
    reached = ~same & ~klass & ~exists                         # the gain is computed from here on
    gain[e[reached]] = g[reached]
    ab[e[~same]] = np.stack([a, b], 1)[~same]
    return status, gain, ab


def flip_apply(faces, T, status, rank, ab, best):
    """-> (faces_out [F, 3], win [E] uint8)"""
    t = T.table
    n_edges = len(t.u)
    a, b = ab[:, 0], ab[:, 1]
    win = (status == CANDIDATE) & (rank < n_edges)
    for x in (t.u, t.v, a, b):
        win &= rank == best[np.maximum(x, 0)]
    out = faces.copy()
    e = np.nonzero(win)[0]
    if len(e):
        f0, f1, _, _, _, _, c0, c1, _ = _children(faces, T, e)
        out[f0], out[f1] = c0, c1
    return out, win.astype(np.uint8)


# ---- relax -----------------------------------------------------------------------------------------------------------------
def relax(pos, faces, T):
    out = pos.copy()
    t = T.table
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(len(pos)):
            ring = ring_of(T, w)
            if T.vclass[w] != 0 or len(ring) == 0:
                continue
            s = pos[ring[0]].copy()
            for x in ring[1:]:
                s = s + pos[x]
            q = s / float(len(ring))
            total = first = None
            for g in T.vedge[T.vedge_off[w]:T.vedge_off[w + 1]]:
                x = t.v[g] if t.u[g] == w else t.u[g]
                if x == w:
                    continue
                ys = []
                for f in (T.face0[g], T.face1[g]):
                    y = [c for c in faces[f] if c != w and c != x] if f >= 0 else []
                    ys.append(int(y[0]) if y else -1)
                if ys[0] >= 0 and ys[1] >= 0 and ys[1] < ys[0]:
                    ys.reverse()
                for y in ys:
                    if y < 0:
                        continue
                    n = _cross(pos[x] - pos[w], pos[y] - pos[w])
                    l2 = _dot(n, n)
                    if not (l2 > 0.0 and l2 < np.inf):
                        continue
                    if total is None:
                        total, first = n.copy(), n
                    elif _dot(n, first) >= 0.0:
                        total = total + n
                    else:
                        total = total - n
            if total is None:
                continue
            l2 = _dot(total, total)
            if not (l2 > 0.0 and l2 < np.inf):
                continue
            nh = total / np.sqrt(l2)
            out[w] = q + _dot(pos[w] - q, nh) * nh
    return out


# ---- the driver ------------------------------------------------------------------------------------------------------------
class Remeshed(NamedTuple):
    verts: np.ndarray
    faces: np.ndarray
    attributes: np.ndarray
    iterations: int
    collapsed: tuple
    flipped: tuple
    split: tuple


RING_PASSES = 2        # passes of vertex_min mode 1 after mode 0: the closed neighbourhoods of two winners share no vertex


def collapse_round(pos, faces, low, high, cos_border, trace=None):
    """one sub-round -> (winners, pos', faces')"""
    T = topo(faces, len(pos))
    status, keep, gone = collapse_check(pos, faces, T, low, high, cos_border)
    if not (status == CANDIDATE).any():
        return 0, pos, faces
    rank = ranks(status, edge_length2(pos, T))
    best = vertex_min(T, faces, status, rank, 0)
    for _ in range(RING_PASSES):
        best = vertex_min(T, faces, status, rank, 1, best)
    remap, pos_out, win = collapse_apply(pos, T, status, rank, keep, gone, best)
    if trace is not None:
        trace(kind="collapse", pos=pos, faces=faces, T=T, status=status, keep=keep, gone=gone, rank=rank, win=win,
              pos_out=pos_out, faces_out=map_faces(faces, remap))
    if not win.any():
        return 0, pos, faces
    return int(win.sum()), pos_out, map_faces(faces, remap)


def flip_round(pos, faces, trace=None):
    T = topo(faces, len(pos))
    status, gain, ab = flip_check(pos, faces, T)
    if not (status == CANDIDATE).any():
        return 0, faces
    rank = ranks(status, -gain.astype(np.int64))
    best = vertex_min(T, faces, status, rank, 2)
    out, win = flip_apply(faces, T, status, rank, ab, best)
    if trace is not None:
        trace(kind="flip", pos=pos, faces=faces, T=T, status=status, gain=gain, ab=ab, rank=rank, win=win, faces_out=out)
    if not win.any():
        return 0, faces
    return int(win.sum()), out


def compact(pos, faces):
    """meshclean.compact_mesh: the vertices no face uses dropped, the others in their order"""
    used = np.zeros(len(pos), bool)
    used[faces.reshape(-1)] = True
    return pos[used], (np.cumsum(used) - 1)[faces]


def moving(T):
    """[V] bool: the vertices relax moves and the projection takes back to the input"""
    return (T.vclass == 0) & (np.diff(T.ring_off) > 0)


def remesh_isotropic(verts, faces, target_edge, iterations=5, project=True, border_angle=30.0, attributes=None,
                     max_subrounds=16, trace=None):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    low, high = 0.8 * target_edge, target_edge * 4 / 3
    cos_border = math.cos(math.radians(border_angle))
    pos = np.asarray(verts, np.float64)
    src_pos, src_faces = pos, faces
    collapsed, flipped, split = [], [], []
    for _ in range(iterations):
        if len(faces) == 0:
            collapsed.append(0), flipped.append(0), split.append(0)
            continue
        s = S.subdivide_to_edge(pos, faces, high)
        split.append(len(s.verts) - len(pos))
        pos, faces = s.verts, s.faces
        if trace is not None:
            trace(kind="split", pos=pos, faces=faces)
        total = 0
        for _ in range(max_subrounds):
            n, pos, faces = collapse_round(pos, faces, low, high, cos_border, trace)
            if n == 0:
                break
            total += n
        collapsed.append(total)
        pos, faces = compact(pos, faces)
        total = 0
        for _ in range(max_subrounds):
            if len(faces) == 0:
                break
            n, faces = flip_round(pos, faces, trace)
            if n == 0:
                break
            total += n
        flipped.append(total)
        if len(faces) == 0:
            continue
        T = topo(faces, len(pos))
        new = relax(pos, faces, T)
        if project:
            rows = np.nonzero(moving(T))[0]
            if len(rows):
                _, face, point, _ = meshdist_ref.closest(new[rows], src_pos, src_faces)
                new[rows[face >= 0]] = point[face >= 0]
        pos = new
        if trace is not None:
            trace(kind="relax", pos=pos, faces=faces)
    attr = None
    if attributes is not None:
        attr = transfer(src_pos, src_faces, np.asarray(attributes), pos)
    return Remeshed(pos.astype(np.asarray(verts).dtype), faces, attr, iterations, tuple(collapsed), tuple(flipped), tuple(split))


def transfer(src_pos, src_faces, attributes, points):
    """meshclean.transfer_attributes: (w0 a0 + w1 a1) + w2 a2 at the closest point of the source"""
    _, face, _, bary = meshdist_ref.closest(points, src_pos, src_faces)
    rows = attributes.astype(np.float64)[src_faces[np.maximum(face, 0)]]
    w = bary[:, :, None]
    out = (w[:, 0] * rows[:, 0] + w[:, 1] * rows[:, 1]) + w[:, 2] * rows[:, 2]
    out[face < 0] = np.nan
    return out.astype(attributes.dtype)


# ---- the test meshes and their measures ------------------------------------------------------------------------------------
def squashed_ico2():
    """meshray_ref.icosphere(2) scaled by (1, 1, 3) and normalised back to the unit sphere: crowded at the equator"""
    v, f = meshray_ref.icosphere(2)
    v = np.array(v, np.float64) * np.array([1.0, 1.0, 3.0])
    return v / np.linalg.norm(v, axis=1)[:, None], np.asarray(f, np.int64)


def jittered_sheet(n=8, seed=3):
    """meshray_ref.grid_sheet(n) with its inner vertices moved in the plane by up to 0.45 of the spacing: collapses that
    would turn a face over"""
    v, f = meshray_ref.grid_sheet(n)
    v, f = np.array(v, np.float64), np.asarray(f, np.int64)
    inner = ~meshsmooth_ref.border_vertices(f, len(v))
    spacing = float(edge_lengths(v, f).min())
    flat = np.ptp(v, 0) > 0
    step = np.random.default_rng(seed).uniform(-0.45, 0.45, v.shape) * spacing * flat
    v[inner] += step[inner]
    return v, f


def dented_disk(n=8):
    """a flat fan of n faces round vertex 0 whose rim vertex 1 is pulled inside the chord of its neighbours: flipping the
    spoke (0, 1) would bring the valences nearer their targets and turn a face over"""
    ang = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang), 0.0 * ang], 1)])
    v[1] *= 0.3
    return v, np.array([(0, 1 + k, 1 + (k + 1) % n) for k in range(n)], np.int64)


def tetrahedron():
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return v, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int64)


def meshes():
    """the nine meshes of the issue, name -> (verts, faces)"""
    out = dict(S.meshes(), squashed_ico2=squashed_ico2())
    return {k: (np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)) for k, (v, f) in out.items()}


def mean_edge(pos, faces):
    return meshsmooth_ref.mean_edge_length(pos, faces)


def edge_lengths(pos, faces):
    e = meshsmooth_ref.unique_edges(faces, len(pos))
    return np.sqrt(_dist2(pos[e[:, 0]], pos[e[:, 1]]))


def quality(pos, faces, target_edge):
    """(share of the edges within [0.8 L, 4/3 L], the smallest and the mean triangle quality 4 sqrt(3) area / sum of the
    squared edges, the standard deviation of the edge lengths over their mean)"""
    length = edge_lengths(pos, faces)
    share = float(((length >= 0.8 * target_edge) & (length <= target_edge * 4 / 3)).mean())
    p0, p1, p2 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
    q = 4.0 * math.sqrt(3.0) * area / (_dist2(p0, p1) + _dist2(p1, p2) + _dist2(p2, p0))
    return share, float(q.min()), float(q.mean()), float(length.std() / length.mean())


def border_edges(faces, n_verts):
    t = S.edge_table(faces, n_verts)
    return int(((t.count == 1) & (t.u != t.v)).sum())


def consistently_wound(faces, n_verts):
    """every edge with two half-edges is run once in each direction"""
    t = S.edge_table(faces, n_verts)
    two = np.nonzero(t.count == 2)[0]
    h0, h1 = t.he_id[t.edge_start[two]], t.he_id[t.edge_start[two] + 1]
    flat = faces.reshape(-1)
    return bool(((flat[h0] == t.u[two]) != (flat[h1] == t.u[two])).all())
