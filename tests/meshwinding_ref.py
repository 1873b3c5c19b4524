"""The numpy restatement of csrc/meshwinding.hip: the linear octree over the faces, the node moments and
the walk, every float64 product, sum, quotient and root in the kernels' order (numpy fuses nothing).  Only atan2 is not
defined to the bit.  The walk is vectorised over the queries the way the kernel is over a wavefront: one pass over the
preorder with a `resume` index per query.  tests/test_meshwinding_ref.py holds it to things it was not built from.

The rules.  A face is absent when an index is out of range, a vertex is not finite or its area vector
A = 1/2 (p1 - p0) x (p2 - p0) has a length sqrt((Ax Ax + Ay Ay) + Az Az) that is zero or not finite.  The leaf cell of a
face is floor((c - lo) / leaf) per axis of its centroid c = (p0 + (p1 + p2)) / 3, lo the lower corner of the box of the
usable faces, clamped into the grid; its key the Morton interleave (x highest).  Faces are sorted by key (stable); the
node of level l is key >> 3 l, l = 0 .. L, L the first level with one node; nodes stand in preorder (first face, level
descending); skip[i] is the first node whose first face is >= node i's end.
Raw moments about lo, with x = c - lo and a = |A|: W = sum a, M = sum a x, S = sum A, T0_jk = sum x_j A_k,
Q0_ijk = sum A_i (x_j x_k + C_jk), C_jk = (d0_j d0_k + (d1_j d1_k + d2_j d2_k)) / 12 with d = p - c; each accumulator
starts at 0.0 and a leaf adds its faces in sorted order, a parent its children in preorder.  Then s = M / W,
centre = lo + s, T_jk = T0_jk - s_j S_k, Q_ijk = ((Q0_ijk - s_k T_ji) - s_j T_ki) - (s_j s_k) S_i, r2 = the squared
distance from the centre to the farthest corner of the box of the node's vertices."""
import numpy as np

FOUR_PI = 4.0 * np.pi
WINDING_LEAF_FACTOR = 2.0          # evaluation.WINDING_LEAF_FACTOR (tests/test_meshwinding_abi.py holds the two equal)
AXIS_CELLS = 1 << 21
SYM = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}


def dot3(x, y, z):
    return (x * x + y * y) + z * z


def vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vcross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def spread3(x):
    x = x.astype(np.uint64) & np.uint64(0x1fffff)
    for s, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3),
                 (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def morton(cx, cy, cz):
    return ((spread3(cx) << np.uint64(2)) | (spread3(cy) << np.uint64(1)) | spread3(cz)).astype(np.int64)


def face_geometry(verts, faces):
    """-> usable [F] bool, corners [F, 3, 3], area vectors [F, 3], their lengths [F], centroids [F, 3] (rows of absent
    faces are meaningless)"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    P = verts[np.where(ok[:, None], faces, 0)]
    with np.errstate(all="ignore"):
        ok &= np.isfinite(P).all((1, 2))
        A = 0.5 * vcross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        a = np.sqrt(dot3(A[:, 0], A[:, 1], A[:, 2]))
        ok &= (a > 0) & (a < np.inf)
        c = (P[:, 0] + (P[:, 1] + P[:, 2])) / 3.0
    return ok, P, A, a, c


def default_leaf(verts, faces, factor=None):
    """factor x the mean longest box side of the faces without a non-finite vertex (MeshIndex's statistic)"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    P = verts[faces]
    P = P[np.isfinite(P).all((1, 2))]
    return (WINDING_LEAF_FACTOR if factor is None else factor) * float((P.max(1) - P.min(1)).max(1).mean())


def leaf_grid(lo, hi, leaf):
    """(leaf, grid): the leaf edge doubles until every axis has at most 2^21 cells"""
    if not leaf > 0:
        ext = max(h - l for l, h in zip(lo, hi))
        leaf = ext if ext > 0 else 1.0
    while True:
        grid = [int(np.floor((h - l) / leaf)) + 1 for l, h in zip(lo, hi)]
        if max(grid) <= AXIS_CELLS:
            return leaf, grid
        leaf *= 2.0


def cell_keys(points, lo, leaf, grid):
    c = np.floor((points - lo) / leaf)
    c = np.clip(c, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    c = np.clip(c, 0, np.asarray(grid, np.int64) - 1)
    return morton(c[:, 0], c[:, 1], c[:, 2])


class Tree:
    """the linear octree of a mesh and its node records; `leaf`: the leaf edge (default_leaf when None)"""

    def __init__(self, verts, faces, leaf=None):
        verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
        self.verts, self.faces = verts, faces
        ok, P, A, a, c = face_geometry(verts, faces)
        finite = ((faces >= 0) & (faces < len(verts))).all(1)
        finite[finite] = np.isfinite(verts[faces[finite]]).all((1, 2))
        box = verts[faces[finite]]
        self.lo, self.hi = box.min((0, 1)), box.max((0, 1))
        self.leaf, self.grid = leaf_grid(self.lo, self.hi, default_leaf(verts, faces) if leaf is None else leaf)
        keys = np.full(len(faces), -1, np.int64)
        keys[ok] = cell_keys(c[ok], self.lo, self.leaf, self.grid)
        order = np.argsort(keys, kind="stable")
        order = order[keys[order] >= 0]
        self.face_keys, self.sorted_faces, skeys = keys, order, keys[order]
        n = len(order)
        first, end, level = [], [], []
        ell = 0
        while n:
            ids = skeys >> (3 * ell)
            start = np.nonzero(np.r_[True, ids[1:] != ids[:-1]])[0]
            first.append(start), end.append(np.r_[start[1:], n]), level.append(np.full(len(start), ell))
            if len(start) == 1:
                break
            ell += 1
        if n == 0:
            first, end, level = [np.zeros(0, np.int64)] * 3, [np.zeros(0, np.int64)] * 3, [np.zeros(0, np.int64)] * 3
        first, end, level = np.concatenate(first), np.concatenate(end), np.concatenate(level)
        pre = np.lexsort((-level, first))
        self.first, self.end, self.level = first[pre], end[pre], level[pre]
        self.skip = np.searchsorted(self.first, self.end, side="left")
        self.n_nodes = len(pre)
        self.is_leaf = self.skip == np.arange(self.n_nodes) + 1
        self._moments(P, A, a, c)

    def _face_raw(self, P, A, a, c):
        """[n sorted faces, 34] the terms a face adds to W, M, S, T0, Q0"""
        f = self.sorted_faces
        P, A, a, c = P[f], A[f], a[f], c[f]
        x = c - self.lo
        d = P - c[:, None, :]
        t = np.zeros((len(f), 34))
        t[:, 0] = a
        for j in range(3):
            t[:, 1 + j] = a * x[:, j]
            t[:, 4 + j] = A[:, j]
            for k in range(3):
                t[:, 7 + 3 * j + k] = x[:, j] * A[:, k]
        for (j, k), p in SYM.items():
            C = (d[:, 0, j] * d[:, 0, k] + (d[:, 1, j] * d[:, 1, k] + d[:, 2, j] * d[:, 2, k])) / 12.0
            xx = x[:, j] * x[:, k] + C
            for i in range(3):
                t[:, 16 + 6 * i + p] = A[:, i] * xx
        return t, P.min(1), P.max(1)

    def _moments(self, P, A, a, c):
        n = self.n_nodes
        raw, blo, bhi = np.zeros((n, 34)), np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
        if n == 0:
            self.raw, self.rec = raw, np.zeros((0, 32))
            return
        terms, flo, fhi = self._face_raw(P, A, a, c)
        leaves = np.nonzero(self.is_leaf)[0]
        count = self.end[leaves] - self.first[leaves]
        for k in range(int(count.max())):                       # the k-th face of every leaf that has one
            sel = leaves[count > k]
            s = self.first[sel] + k
            raw[sel] = raw[sel] + terms[s]
            blo[sel], bhi[sel] = np.minimum(blo[sel], flo[s]), np.maximum(bhi[sel], fhi[s])
        for ell in range(1, int(self.level.max()) + 1):         # the k-th child of every node of the level
            nodes = np.nonzero(self.level == ell)[0]
            child = nodes + 1
            live = np.ones(len(nodes), bool)
            for k in range(8):
                live &= child < self.skip[nodes]
                if not live.any():
                    break
                p, ch = nodes[live], child[live]
                raw[p] = raw[p] + raw[ch]
                blo[p], bhi[p] = np.minimum(blo[p], blo[ch]), np.maximum(bhi[p], bhi[ch])
                child = np.where(live, self.skip[np.minimum(child, n - 1)], child)
        self.raw, self.box_lo, self.box_hi = raw, blo, bhi
        rec = np.zeros((n, 32))
        s = raw[:, 1:4] / raw[:, 0:1]
        S = raw[:, 4:7]
        T = np.zeros((n, 3, 3))
        for j in range(3):
            for k in range(3):
                T[:, j, k] = raw[:, 7 + 3 * j + k] - s[:, j] * S[:, k]
        centre = self.lo + s
        ext = np.maximum(centre - blo, bhi - centre)
        rec[:, 0:3], rec[:, 3], rec[:, 4:7] = centre, dot3(ext[:, 0], ext[:, 1], ext[:, 2]), S
        for k in range(3):
            rec[:, 7 + k] = T[:, k, k]
        rec[:, 10], rec[:, 11], rec[:, 12] = T[:, 0, 1] + T[:, 1, 0], T[:, 0, 2] + T[:, 2, 0], T[:, 1, 2] + T[:, 2, 1]
        for i in range(3):
            for (j, k), p in SYM.items():
                rec[:, 13 + 6 * i + p] = ((raw[:, 16 + 6 * i + p] - s[:, k] * T[:, j, i]) - s[:, j] * T[:, k, i]) \
                    - (s[:, j] * s[:, k]) * S[:, i]
        rec[:, 31] = (T[:, 0, 0] + T[:, 1, 1]) + T[:, 2, 2]
        self.rec, self.T = rec, T


def expansion(rec, r, d2):
    """the order-2 expansion of node record rec [32] along r [M, 3], d2 = |r|^2 [M] -> (term 0, term 1, term 2)"""
    d = np.sqrt(d2)
    d3 = d2 * d
    d5 = d3 * d2
    d7 = d5 * d2
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    t0 = ((rec[4] * x + rec[5] * y) + rec[6] * z) / d3
    rTr = ((rec[7] * xx + rec[8] * yy) + rec[9] * zz) + ((rec[10] * xy + rec[11] * xz) + rec[12] * yz)
    t1 = rec[31] / d3 - (3.0 * rTr) / d5
    g, H = [], []
    for i in range(3):
        Q = rec[13 + 6 * i:19 + 6 * i]
        g.append(((Q[0] * xx + Q[3] * yy) + Q[5] * zz) + 2.0 * ((Q[1] * xy + Q[2] * xz) + Q[4] * yz))
        H.append((Q[0] + Q[3]) + Q[5])
    cubic = (x * g[0] + y * g[1]) + z * g[2]
    V0 = (rec[13 + 0] + rec[19 + 1]) + rec[25 + 2]
    V1 = (rec[13 + 1] + rec[19 + 3]) + rec[25 + 4]
    V2 = (rec[13 + 2] + rec[19 + 4]) + rec[25 + 5]
    lin = 2.0 * ((V0 * x + V1 * y) + V2 * z) + ((H[0] * x + H[1] * y) + H[2] * z)
    t2 = 0.5 * ((-3.0 * lin) / d5 + (15.0 * cubic) / d7)
    return t0, t1, t2


def solid_angle(P, q):
    """van Oosterom-Strackee: corners P [..., 3, 3] seen from q [..., 3] -> the solid angle, 0 where num == 0"""
    a, b, c = P[..., 0, :] - q, P[..., 1, :] - q, P[..., 2, :] - q
    la, lb, lc = (np.sqrt(dot3(v[..., 0], v[..., 1], v[..., 2])) for v in (a, b, c))
    num = vdot(a, vcross(b, c))
    den = (la * (lb * lc) + vdot(b, c) * la) + (vdot(a, b) * lc + vdot(c, a) * lb)
    return np.where(num == 0.0, 0.0, 2.0 * np.arctan2(num, den))


def winding(tree, points, beta=2.0, order=2):
    """-> dict(w [M], exact [M] faces evaluated exactly, far [M] nodes replaced, abs [M] the sum of |term|): the walk
    of DESIGN.md 4.22 for every query, one accumulator each.  `order` < 2 leaves the higher terms out (the design
    table only; the kernel has order 2)."""
    q = np.asarray(points, np.float64).reshape(-1, 3)
    M, n = len(q), tree.n_nodes
    acc, mag = np.zeros(M), np.zeros(M)
    n_exact, n_far = np.zeros(M, np.int64), np.zeros(M, np.int64)
    resume = np.zeros(M, np.int64)
    with np.errstate(all="ignore"):
        beta2 = np.float64(beta) * np.float64(beta)
        corners = tree.verts[tree.faces[tree.sorted_faces]]
        i = 0
        while i < n and M:
            part = np.nonzero(resume <= i)[0]
            rec = tree.rec[i]
            r = rec[0:3] - q[part]
            d2 = dot3(r[:, 0], r[:, 1], r[:, 2])
            far = d2 > beta2 * rec[3]
            pf, pn = part[far], part[~far]
            if len(pf):
                t0, t1, t2 = expansion(rec, r[far], d2[far])
                e = (t0 + t1) + t2 if order == 2 else (t0 + t1 if order == 1 else t0)
                acc[pf] = acc[pf] + e
                mag[pf] += np.abs(e)
                n_far[pf] += 1
                resume[pf] = tree.skip[i]
            if tree.is_leaf[i]:
                for s in range(tree.first[i], tree.end[i]):
                    term = solid_angle(corners[s], q[pn])
                    acc[pn] = acc[pn] + term
                    mag[pn] += np.abs(term)
                n_exact[pn] += tree.end[i] - tree.first[i]
                resume[pn] = tree.skip[i]
                i = int(resume.min())
            elif len(pn):
                i += 1
            else:
                i = max(int(resume.min()), i + 1)
    return dict(w=acc / FOUR_PI, exact=n_exact, far=n_far, abs=mag / FOUR_PI)


def brute(verts, faces, points):
    """an independent exact sum: every usable face in face order, no tree"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    ok = face_geometry(verts, faces)[0]
    q = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        om = solid_angle(verts[faces[ok]][None], q[:, None, :])
    return om.sum(1) / FOUR_PI


# ---- the meshes the CPU and GPU tests share ---------------------------------------------------------------------------
def moebius(nu=48, nv=4):
    """a Moebius band: one-sided, so its faces cannot be wound consistently"""
    u = np.arange(nu) * (2 * np.pi / nu)
    t = np.linspace(-0.3, 0.3, nv + 1)

    def pt(iu, it):
        if iu == nu:
            iu, it = 0, nv - it
        a, s = u[iu], t[it]
        return ((1 + s * np.cos(a / 2)) * np.cos(a), (1 + s * np.cos(a / 2)) * np.sin(a), s * np.sin(a / 2))
    index, v, f = {}, [], []

    def vid(iu, it):
        if iu == nu:
            iu, it = 0, nv - it
        if (iu, it) not in index:
            index[(iu, it)] = len(v)
            v.append(pt(iu, it))
        return index[(iu, it)]
    for iu in range(nu):
        for it in range(nv):
            a, b, c, d = vid(iu, it), vid(iu + 1, it), vid(iu + 1, it + 1), vid(iu, it + 1)
            f += [(a, b, c), (a, c, d)]
    return np.array(v, np.float64), np.array(f, np.int64)


def fan(n=96, radius=1.0, hub_radius=0.004):
    """a disc of n slivers around a hub, plus n tiny faces at the hub itself: far more than 64 faces share the hub's leaf"""
    a = np.arange(n) * (2 * np.pi / n)
    rim = np.stack([radius * np.cos(a), radius * np.sin(a), 0.05 * np.sin(3 * a)], 1)
    inner = np.stack([hub_radius * np.cos(a), hub_radius * np.sin(a), np.zeros(n)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.0]], inner, rim])
    f = [(0, 1 + k, 1 + (k + 1) % n) for k in range(n)]
    for k in range(n):
        i0, i1, r0, r1 = 1 + k, 1 + (k + 1) % n, 1 + n + k, 1 + n + (k + 1) % n
        f += [(i0, r0, r1), (i0, r1, i1)]
    return v, np.array(f, np.int64)


def two_sheets(n=16):
    """two rippled open sheets of n x n quads one above the other, the upper one wound the other way"""
    import meshray_ref
    v0, f0 = meshray_ref.grid_sheet(n, lambda x, y: 0.05 * np.sin(5.0 * x) * np.cos(3.0 * y))
    v1, f1 = meshray_ref.grid_sheet(n, lambda x, y: 0.3 + 0.04 * np.cos(4.0 * x + y))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1[:, [0, 2, 1]] + len(v0)])


def with_absent_faces(v, f):
    """the mesh plus a face with a NaN vertex, a face of zero area and a face with an index out of range is not possible
    through the drivers (they refuse it): the first two only, put in front so that every face index moves"""
    v = np.concatenate([v, [[np.nan, 0.0, 0.0]]])
    bad = np.array([[0, 1, len(v) - 1], [2, 2, 3], [4, 5, 4]], np.int64)
    return v, np.concatenate([bad, f])


def punched_sphere(subdivisions=3, radius=0.6, fraction=0.08, seed=0):
    """an icosphere with `fraction` of its faces removed by a seeded permutation"""
    import meshray_ref
    v, f = meshray_ref.icosphere(subdivisions, radius)
    keep = np.sort(np.random.default_rng(seed).permutation(len(f))[int(round(fraction * len(f))):])
    return v, f[keep]


def shell_points(subdivisions, radius, radii):
    """the vertices of an icosphere scaled to each radius of `radii`"""
    import meshray_ref
    v = meshray_ref.icosphere(subdivisions, 1.0)[0]
    return np.concatenate([v * (radius * r) for r in radii])
