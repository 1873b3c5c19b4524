"""numpy / plain-Python float64 restatement of csrc/meshhole.hip and of meshclean.border_loops / close_holes, operation by
operation (include/nudf.h states the definitions).  Python's float is an IEEE double and never contracts a product into a
sum; math.sqrt is correctly rounded.  Loops are extracted twice: by a plain walk along the links (`loops`, the
definition) and through the pointer-doubling rounds with the package's glue restated (`loops_from_rank`); the tests hold
the two against each other.  Faces are taken to be in range: the host checks them."""
import math
from typing import NamedTuple

import numpy as np

import meshsubdiv_ref

FILLED, OPEN_CHAIN, TOO_MANY_EDGES, PERIMETER, NONFINITE, DUPLICATE, REPEATED_VERTEX = range(7)
MAX_HOLE_EDGES = 64
FAN_CAP = 4096


class Table(NamedTuple):
    u: np.ndarray            # [E] the smaller end
    v: np.ndarray            # [E] the larger end; rows ordered by (u, v)
    count: np.ndarray        # [E] half-edges on the edge
    face0: np.ndarray        # [E] face of the first half-edge
    face1: np.ndarray        # [E] face of the second, or -1
    he_edge: np.ndarray      # [3 F]
    key: np.ndarray          # [E] u V + v
    bedge: np.ndarray        # [B] the rows with count 1
    brank: np.ndarray        # [E] position in bedge, or -1


def table(faces, n_verts):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = meshsubdiv_ref.edge_table(f, n_verts)
    face0 = t.he_id[t.edge_start] // 3 if len(t.u) else np.zeros(0, np.int64)
    face1 = np.full(len(t.u), -1, np.int64)
    two = t.count >= 2
    face1[two] = t.he_id[t.edge_start[two] + 1] // 3
    bedge = np.nonzero(t.count == 1)[0].astype(np.int64)
    brank = np.full(len(t.u), -1, np.int64)
    brank[bedge] = np.arange(len(bedge))
    return Table(t.u, t.v, t.count, face0, face1, t.he_edge, t.u * max(n_verts, 1) + t.v, bedge, brank)


# ---- link -----------------------------------------------------------------------------------------------------------------
def _other_edge_at(tb, f, tri, v, frm):
    found = [tb.he_edge[3 * f + k] for k in range(3) if (tri[k] == v or tri[(k + 1) % 3] == v) and tb.he_edge[3 * f + k] != frm]
    return int(found[0]) if len(found) == 1 else -1


def link(faces, tb):
    """[2 B]: the partner state of (border edge b, end) = 2 b + end, or -1 for a blocked end"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.full(2 * len(tb.bedge), -1, np.int64)
    for s in range(len(out)):
        e0 = int(tb.bedge[s >> 1])
        v = int((tb.u, tb.v)[s & 1][e0])
        f0 = int(tb.face0[e0])
        cur, e = f0, e0
        for _ in range(FAN_CAP):
            tri = f[cur]
            if tri[0] == tri[1] or tri[1] == tri[2] or tri[0] == tri[2]:
                break
            ne = _other_edge_at(tb, cur, tri, v, e)
            if ne < 0:
                break
            if tb.count[ne] == 1:
                if ne != e0 and tb.u[ne] != tb.v[ne]:
                    out[s] = 2 * tb.brank[ne] + (1 if tb.v[ne] == v else 0)
                break
            if tb.count[ne] != 2:
                break
            nf = int(tb.face1[ne]) if tb.face0[ne] == cur else (int(tb.face0[ne]) if tb.face1[ne] == cur else -1)
            if nf == f0 or nf == cur or nf < 0:
                break
            cur, e = nf, ne
    return out


# ---- rank -----------------------------------------------------------------------------------------------------------------
def successor(lnk):
    """across the edge, then along the link; at a blocked end back along the chain"""
    s = np.arange(len(lnk), dtype=np.int64)
    over = lnk[s ^ 1] if len(lnk) else lnk
    return np.where(over >= 0, over, s ^ 1)


def rank_init(lnk):
    s = np.arange(len(lnk), dtype=np.int64)
    return np.stack([successor(lnk), s, np.zeros_like(s)], 1)


def rank_rounds(n_border):
    return (2 * n_border - 1).bit_length() + 1 if n_border > 0 else 0


def rank_round(tab, r):
    j = tab[:, 0]
    nxt = tab[j]
    less = nxt[:, 1] < tab[:, 1]
    return np.stack([nxt[:, 0], np.where(less, nxt[:, 1], tab[:, 1]), np.where(less, (1 << r) + nxt[:, 2], tab[:, 2])], 1)


def rank(lnk):
    tab = rank_init(lnk)
    for r in range(rank_rounds(len(lnk) // 2)):
        tab = rank_round(tab, r)
    return tab


# ---- loops ----------------------------------------------------------------------------------------------------------------
class Loops(NamedTuple):
    loop_off: np.ndarray     # [L + 1]
    loop_vertex: np.ndarray  # the vertex at which each edge is entered, in canonical order
    loop_edge: np.ndarray    # rows of the edge table, same CSR
    closed: np.ndarray       # [L] bool
    edge_loop: np.ndarray    # [E] loop of each border edge, -1 otherwise


def _pack(tb, per_loop):
    """per_loop: [(smallest border index, closed, [directed states])] -> Loops, ordered by smallest border index"""
    per_loop = sorted(per_loop, key=lambda t: t[0])
    off, vert, edge, closed = [0], [], [], []
    edge_loop = np.full(len(tb.u), -1, np.int64)
    for l, (_, c, states) in enumerate(per_loop):
        for s in states:
            e = int(tb.bedge[s >> 1])
            edge.append(e)
            vert.append(int((tb.u, tb.v)[s & 1][e]))
            edge_loop[e] = l
        off.append(len(edge))
        closed.append(c)
    return Loops(np.array(off, np.int64), np.array(vert, np.int64), np.array(edge, np.int64), np.array(closed, bool),
                 edge_loop)


def loops(tb, lnk):
    """the definition, by a walk: a closed loop starts at its smallest directed state; a chain at the one of its two
    blocked ends' states that is smaller"""
    n = len(lnk)
    seen = np.zeros(n // 2, bool)
    found = []
    for s0 in range(n):
        if seen[s0 >> 1]:
            continue
        # back along the links to a blocked end, or around once
        s, is_closed = s0, False
        while lnk[s] >= 0:
            s = int(lnk[s]) ^ 1
            if s == s0:
                is_closed = True
                break
        if is_closed:
            start = s0                                        # s0 ascends: the first state met on a loop is its smallest
        else:
            t = s
            while lnk[t ^ 1] >= 0:
                t = int(lnk[t ^ 1])
            start = min(s, t ^ 1)
        states, s = [], start
        while True:
            states.append(s)
            seen[s >> 1] = True
            nx = int(lnk[s ^ 1])
            if nx < 0 or nx == start:
                break
            s = nx
        found.append((min(x >> 1 for x in states), is_closed, states))
    return _pack(tb, found)


def loops_from_rank(tb, lnk, tab):
    """the package's glue: every state lies on a cycle, m = its smallest state and d the steps to it"""
    n = len(lnk)
    s = np.arange(n, dtype=np.int64)
    m, d = tab[:, 1], tab[:, 2]
    chain = m == m[s ^ 1]
    length = np.bincount(m, minlength=n)[m]
    first = np.full(n, n, np.int64)
    starts = s[lnk < 0]
    np.minimum.at(first, m[starts], starts)
    origin = np.where(chain, first[m], m)
    origin = np.where(origin < n, origin, m)
    pos = (d[origin] - d) % length
    canonical = np.where(chain, 2 * pos < length, m < m[s ^ 1])
    label = np.minimum(m, m[s ^ 1]) >> 1
    cs = s[canonical]
    cs = cs[np.argsort(pos[cs], kind="stable")]
    cs = cs[np.argsort(label[cs], kind="stable")]
    per = {}
    for x in cs:
        per.setdefault(int(label[x]), (int(label[x]), not chain[x], []))[2].append(int(x))
    return _pack(tb, list(per.values()))


# ---- count ----------------------------------------------------------------------------------------------------------------
def _length(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def count(pos, tb, lp, max_edges, max_perimeter=None):
    """-> (perimeter [L], status [L] int8, new_count [L])"""
    pos = np.asarray(pos, np.float64)
    bound = math.inf if max_perimeter is None else float(max_perimeter)
    L = len(lp.closed)
    per, status, cnt = np.zeros(L), np.zeros(L, np.int8), np.zeros(L, np.int64)
    for l in range(L):
        b, e = int(lp.loop_off[l]), int(lp.loop_off[l + 1])
        n, total, finite = e - b, 0.0, True
        for i in range(b, e):
            p, q = pos[tb.u[lp.loop_edge[i]]].tolist(), pos[tb.v[lp.loop_edge[i]]].tolist()
            finite = finite and all(map(math.isfinite, p + q + pos[lp.loop_vertex[i]].tolist()))
            ln = _length(p, q)
            total = ln if i == b else total + ln
        vs = lp.loop_vertex[b:e]
        if not lp.closed[l]:
            st = OPEN_CHAIN
        elif n < 3 or n > max_edges:
            st = TOO_MANY_EDGES
        elif len(set(vs.tolist())) != n:
            st = REPEATED_VERTEX
        elif not finite or not math.isfinite(total):
            st = NONFINITE
        elif total > bound:
            st = PERIMETER
        else:
            st = FILLED
        per[l], status[l], cnt[l] = total, st, n - 2 if st == FILLED else 0
    return per, status, cnt


# ---- triangulate -----------------------------------------------------------------------------------------------------------
def area(p, q, r):
    """0.5 sqrt(|(q - p) x (r - p)|^2) with np.cross's order of operations"""
    ax, ay, az = q[0] - p[0], q[1] - p[1], q[2] - p[2]
    bx, by, bz = r[0] - p[0], r[1] - p[1], r[2] - p[2]
    cx, cy, cz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    return 0.5 * math.sqrt((cx * cx + cy * cy) + cz * cz)


def min_area(P):
    """P: n points -> (W, split): W[i][j] the least area of a triangulation of v_i ... v_j, k ascending, the first strictly
    smaller value wins"""
    P = [list(map(float, p)) for p in P]
    n = len(P)
    W = [[0.0] * n for _ in range(n)]
    split = [[0] * n for _ in range(n)]
    for d in range(2, n):
        for i in range(n - d):
            j = i + d
            best, arg = None, i + 1
            for k in range(i + 1, j):
                w = (W[i][k] + W[k][j]) + area(P[i], P[k], P[j])
                if best is None or w < best:
                    best, arg = w, k
            W[i][j], split[i][j] = best, arg
    return W, split


def preorder(split, n):
    """the n - 2 triangles (i, k, j) from (0, n - 1): the triangle, then (i, k), then (k, j)"""
    out, stack = [], [(0, n - 1)]
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        k = split[i][j]
        out.append((i, k, j))
        stack.append((k, j))
        stack.append((i, k))
    return out


def triangulate(pos, faces, tb, lp, status, cnt):
    """-> (new_faces [n_new, 3] with the rows of a refused loop -1, status' with DUPLICATE for those)"""
    pos = np.asarray(pos, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    status = status.copy()
    off = np.cumsum(cnt) - cnt
    new = np.full((int(cnt.sum()), 3), -1, np.int64)
    keys = set(tb.key.tolist())
    V = max(len(pos), 1)
    for l in np.nonzero(status == FILLED)[0]:
        b, e = int(lp.loop_off[l]), int(lp.loop_off[l + 1])
        n = e - b
        vs, es = lp.loop_vertex[b:e], lp.loop_edge[b:e]
        _, split = min_area(pos[vs])
        tris = preorder(split, n)
        refused = False
        for i, k, j in tris:
            if (i, j) != (0, n - 1):
                u, v = int(vs[i]), int(vs[j])
                refused = refused or min(u, v) * V + max(u, v) in keys
            elif n == 3:
                refused = refused or tb.face0[es[0]] == tb.face0[es[1]] == tb.face0[es[2]]
        if refused:
            status[l] = DUPLICATE
            continue
        same = 0
        for i in range(n):
            fc = int(tb.face0[es[i]])
            k = [k for k in range(3) if tb.he_edge[3 * fc + k] == es[i]][-1]
            same += int(f[fc][k] == vs[i])
        flip = 2 * same > n
        for t, (i, k, j) in enumerate(tris):
            new[off[l] + t] = (vs[i], vs[j], vs[k]) if flip else (vs[i], vs[k], vs[j])
    return new, status


def shared_diagonals(new, face_loop, n_verts):
    """the loops whose patch has an edge that the patch of a loop with a smaller id has too"""
    V = max(n_verts, 1)
    a, b = new.reshape(-1), np.roll(new, -1, 1).reshape(-1)
    key = np.minimum(a, b) * V + np.maximum(a, b)
    lp = np.repeat(face_loop, 3)
    order = np.argsort(key, kind="stable")
    sk, sl = key[order], lp[order]
    first = np.ones(len(sk), bool)
    first[1:] = sk[1:] != sk[:-1]
    owner = sl[first][np.cumsum(first) - 1] if len(sk) else sl
    return np.unique(sl[sl != owner])


class Closed(NamedTuple):
    faces: np.ndarray
    new_face_loop: np.ndarray
    status: np.ndarray
    loops: Loops
    perimeter: np.ndarray


def close_holes(verts, faces, max_edges=32, max_perimeter=None):
    pos = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tb = table(f, len(pos))
    lnk = link(f, tb)
    lp = loops(tb, lnk)
    per, status, cnt = count(pos, tb, lp, max_edges, max_perimeter)
    new, status = triangulate(pos, f, tb, lp, status, cnt)
    face_loop = np.repeat(np.arange(len(cnt)), cnt)
    keep = new[:, 0] >= 0
    new, face_loop = new[keep], face_loop[keep]
    bad = shared_diagonals(new, face_loop, len(pos))
    status[bad] = DUPLICATE
    keep = ~np.isin(face_loop, bad)
    return Closed(np.concatenate([f, new[keep]]), face_loop[keep], status, lp, per)
