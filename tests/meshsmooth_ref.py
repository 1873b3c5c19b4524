"""numpy float64 restatement of csrc/meshsmooth.hip and of meshclean.smooth_mesh / denoise_mesh, operation by operation and
in the kernels' sum orders: ragged sums run rank by rank (the r-th entry of every list is added in pass r), which is the
list order inside each item.  numpy does not contract a product into a sum; the exp of the bilateral weight is math.exp
(the C library's), one call per (face, neighbour).  Faces are taken to be in range: the host checks them."""
import math

import numpy as np


# ---- topology -------------------------------------------------------------------------------------------------------
def adjacency_sets(faces, n_verts):
    """the one-ring of every vertex as a set: the other ends of the edges of its faces (a repeated vertex is no edge)"""
    ring = [set() for _ in range(n_verts)]
    for t in np.asarray(faces, np.int64).reshape(-1, 3):
        for k in range(3):
            u, w = int(t[k]), int(t[(k + 1) % 3])
            if u != w:
                ring[u].add(w)
                ring[w].add(u)
    return ring


def vertex_adjacency(faces, n_verts):
    """-> (off [V + 1], nbr): the sets above as a CSR, neighbours ascending"""
    ring = adjacency_sets(faces, n_verts)
    off = np.zeros(n_verts + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in ring])
    nbr = np.array([w for r in ring for w in sorted(r)], np.int64)
    return off, nbr


def corners(faces, n_verts):
    """-> (corner_off [V + 1], corner [3 F]): the corners 3 f + k by vertex, ascending inside each"""
    flat = np.asarray(faces, np.int64).reshape(-1)
    corner = np.argsort(flat, kind="stable").astype(np.int64)
    off = np.zeros(n_verts + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(flat, minlength=n_verts))
    return off, corner


def border_vertices(faces, n_verts):
    """[V] bool: the vertex lies on an undirected edge that exactly one half-edge runs along"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, 1).reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key, inv, count = np.unique(lo * max(n_verts, 1) + hi, return_inverse=True, return_counts=True)
    single = count[inv.reshape(-1)] == 1
    out = np.zeros(n_verts, bool)
    out[lo[single]] = True
    out[hi[single]] = True
    return out


def unique_edges(faces, n_verts):
    """[E, 2] the undirected edges u < v, ordered by (u, v)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, 1).reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * max(n_verts, 1) + hi)[lo != hi])
    return np.stack([key // max(n_verts, 1), key % max(n_verts, 1)], 1)


def mean_edge_length(pos, faces):
    e = unique_edges(faces, len(pos))
    d = pos[e[:, 0]] - pos[e[:, 1]]
    d2 = d * d
    return float(np.mean(np.sqrt((d2[:, 0] + d2[:, 1]) + d2[:, 2])))


def face_neighbours(faces, n_verts):
    """for every face the faces that share a vertex with it, in the kernel's visiting order: its vertices in ascending
    index, the corners of each in list order, without the face itself and without a face that holds a vertex visited
    earlier -> list of lists"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    off, corner = corners(f, n_verts)
    out = []
    for i, t in enumerate(f):
        u = sorted(int(x) for x in t)
        row = []
        for q in range(3):
            for h in corner[off[u[q]]:off[u[q] + 1]]:
                j = int(h) // 3
                if j == i or any(u[r] in f[j] for r in range(q)):
                    continue
                row.append(j)
        out.append(row)
    return out


def _padded(rows):
    k = max([len(r) for r in rows], default=0)
    out = np.full((len(rows), k), -1, np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


# ---- arithmetic, in the kernels' grouping ------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _positive_finite(x):
    return (x > 0.0) & (x < np.inf)


def _cot(c, x, y):
    """cot of the angle at c between x - c and y - c, and whether the cross product's length is positive and finite"""
    u, v = x - c, y - c
    n = _cross(u, v)
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot(n, n))
        return _dot(u, v) / length, _positive_finite(length)


def _centres(pos, f):
    return (pos[f[:, 0]] + (pos[f[:, 1]] + pos[f[:, 2]])) / 3.0


def laplace_step(pos, faces, step, weights="uniform", fixed=None, topo=None):
    """one Jacobi step of nudf_meshsmooth_laplace -> pos' [V, 3]"""
    pos, f = np.asarray(pos, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(pos)
    s, W = np.zeros((n, 3)), np.zeros(n)
    if weights == "uniform":
        off, nbr = topo if topo is not None else vertex_adjacency(f, n)
        deg = off[1:] - off[:-1]
        for r in range(int(deg.max()) if n else 0):
            sel = np.nonzero(deg > r)[0]
            s[sel] = s[sel] + pos[nbr[off[sel] + r]]
        W = deg.astype(np.float64)
    else:
        off, corner = topo if topo is not None else corners(f, n)
        deg = off[1:] - off[:-1]
        for r in range(int(deg.max()) if n else 0):
            sel = np.nonzero(deg > r)[0]
            h = corner[off[sel] + r]
            t, k = f[h // 3], h % 3
            rows = np.arange(len(sel))
            pc, pa, pb = pos[t[rows, k]], pos[t[rows, (k + 1) % 3]], pos[t[rows, (k + 2) % 3]]
            cot_b, ok_b = _cot(pb, pc, pa)
            cot_a, ok_a = _cot(pa, pb, pc)
            ok = ok_b & ok_a
            wa = 0.5 * np.where(cot_b > 0.0, cot_b, 0.0)
            wb = 0.5 * np.where(cot_a > 0.0, cot_a, 0.0)
            with np.errstate(all="ignore"):
                new = (s[sel] + wa[:, None] * pa) + wb[:, None] * pb
            s[sel] = np.where(ok[:, None], new, s[sel])
            W[sel] = np.where(ok, W[sel] + (wa + wb), W[sel])
    move = _positive_finite(W)
    if fixed is not None:
        move &= ~np.asarray(fixed, bool)
    with np.errstate(all="ignore"):
        out = pos + step * (s / W[:, None] - pos)
    return np.where(move[:, None], out, pos)


def frames(pos, faces):
    """nudf_meshsmooth_frames -> (normals [F, 3], areas [F], centres [F, 3])"""
    pos, f = np.asarray(pos, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    n = _cross(pos[f[:, 1]] - pos[f[:, 0]], pos[f[:, 2]] - pos[f[:, 0]])
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot(n, n))
        unit = np.where(_positive_finite(length)[:, None], n / length[:, None], 0.0)
    return unit, 0.5 * length, _centres(pos, f)


def normals_step(fnormal, area, centre, inv2sc, inv2ss, neighbours, stats=None):
    """one step of nudf_meshsmooth_normals -> fnormal' [F, 3].  `neighbours`: face_neighbours(...).  `stats`: a dict that
    receives k (the longest neighbour list) and rho (the smallest |s| / sum of w over the faces that changed)"""
    nb = _padded(neighbours)
    s, wsum = np.zeros_like(fnormal), np.zeros(len(fnormal))
    zero = (fnormal == 0.0).all(1)
    for r in range(nb.shape[1]):
        sel = np.nonzero((nb[:, r] >= 0) & ~zero)[0]
        j = nb[sel, r]
        use = ~zero[j]
        ni, nj = fnormal[sel], fnormal[j]
        mj = np.where((_dot(ni, nj) >= 0.0)[:, None], nj, -nj)
        dc, dn = centre[sel] - centre[j], ni - mj
        arg = _dot(dc, dc) * inv2sc + _dot(dn, dn) * inv2ss
        w = area[j] * np.array([math.exp(-x) for x in arg], np.float64).reshape(arg.shape)
        s[sel] = np.where(use[:, None], s[sel] + w[:, None] * mj, s[sel])
        wsum[sel] = np.where(use, wsum[sel] + w, wsum[sel])
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot(s, s))
        ok = _positive_finite(length) & ~zero
        out = np.where(ok[:, None], s / length[:, None], fnormal)
    if stats is not None:
        stats["k"] = max(stats.get("k", 0), nb.shape[1])
        if ok.any():
            stats["rho"] = min(stats.get("rho", np.inf), float((length[ok] / wsum[ok]).min()))
    return out


def update_step(pos, faces, fnormal, fixed=None, topo=None):
    """one Jacobi step of nudf_meshsmooth_update -> pos' [V, 3]"""
    pos, f = np.asarray(pos, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(pos)
    off, corner = topo if topo is not None else corners(f, n)
    deg = off[1:] - off[:-1]
    centre = _centres(pos, f)
    zero = (fnormal == 0.0).all(1)
    s, count = np.zeros((n, 3)), np.zeros(n, np.int64)
    for r in range(int(deg.max()) if n else 0):
        sel = np.nonzero(deg > r)[0]
        j = corner[off[sel] + r] // 3
        use = ~zero[j]
        nf = fnormal[j]
        d = _dot(nf, centre[j] - pos[sel])
        s[sel] = np.where(use[:, None], s[sel] + nf * d[:, None], s[sel])
        count[sel] += use
    move = count > 0
    if fixed is not None:
        move &= ~np.asarray(fixed, bool)
    with np.errstate(all="ignore"):
        out = pos + s / count.astype(np.float64)[:, None]
    return np.where(move[:, None], out, pos)


# ---- drivers --------------------------------------------------------------------------------------------------------
def _fixed_mask(faces, n_verts, boundary, fixed):
    mask = np.zeros(n_verts, bool) if fixed is None else np.asarray(fixed, bool).copy()
    if boundary == "fixed":
        mask |= border_vertices(faces, n_verts)
    return mask


def smooth_mesh(verts, faces, iterations=10, lam=0.5, mu=-0.53, weights="uniform", boundary="fixed", fixed=None):
    dtype = np.asarray(verts).dtype
    pos, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0 or len(pos) == 0 or iterations == 0:
        return np.asarray(verts)
    mask = _fixed_mask(f, len(pos), boundary, fixed)
    topo = vertex_adjacency(f, len(pos)) if weights == "uniform" else corners(f, len(pos))
    for _ in range(iterations):
        pos = laplace_step(pos, f, lam, weights, mask, topo)
        if mu != 0:
            pos = laplace_step(pos, f, mu, weights, mask, topo)
    return pos.astype(dtype)


def denoise_mesh(verts, faces, normal_iterations=5, vertex_iterations=10, sigma_s=0.35, sigma_c=None, boundary="fixed",
                 fixed=None, stats=None):
    dtype = np.asarray(verts).dtype
    pos, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0 or len(pos) == 0:
        return np.asarray(verts), np.zeros((len(f), 3), dtype)
    fn, area, centre = frames(pos, f)
    if sigma_c is None:
        sigma_c = mean_edge_length(pos, f)
    inv2sc, inv2ss = 1.0 / (2.0 * sigma_c * sigma_c), 1.0 / (2.0 * sigma_s * sigma_s)
    nb = face_neighbours(f, len(pos)) if normal_iterations else None
    for _ in range(normal_iterations):
        fn = normals_step(fn, area, centre, inv2sc, inv2ss, nb, stats)
    mask = _fixed_mask(f, len(pos), boundary, fixed)
    topo = corners(f, len(pos))
    for _ in range(vertex_iterations):
        pos = update_step(pos, f, fn, mask, topo)
    return pos.astype(dtype), fn.astype(dtype)


# ---- the test meshes ---------------------------------------------------------------------------------------------------
def cube_mesh(n=8):
    """the surface of [-1, 1]^3 with n x n quads per side and shared vertices, wound outward ->
    (verts, faces, side normal of each face [F, 3])"""
    index, verts, faces, side = {}, [], [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append([2.0 * c / n - 1.0 for c in p])
        return index[p]
    for axis in range(3):
        for s in (0, n):
            a1, a2 = (axis + 1) % 3, (axis + 2) % 3
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[a1], p[a2] = s, i + di, j + dj
                        q.append(vid(tuple(p)))
                    if s == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
                    nrm = [0.0, 0.0, 0.0]
                    nrm[axis] = 1.0 if s else -1.0
                    side += [nrm, nrm]
    return np.array(verts, np.float64), np.array(faces, np.int64), np.array(side, np.float64)


def fan_mesh(n=40):
    """n faces round vertex 0, closed, slightly conical"""
    ang = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.05 * np.cos(3.0 * ang)], 1)])
    f = np.array([(0, 1 + k, 1 + (k + 1) % n) for k in range(n)], np.int64)
    return v, f


def three_on_an_edge():
    """three faces on the edge (0, 1): not a manifold"""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.1], [0.5, -0.6, 0.8], [0.4, -0.5, -0.9]])
    return v, np.array([(0, 1, 2), (1, 0, 3), (0, 1, 4)], np.int64)


def awkward_mesh():
    """a small sheet with an isolated vertex (16), a zero-area face, a face with a repeated vertex, and a vertex (17)
    whose faces are all degenerate"""
    k = np.arange(4) / 3.0
    x, y = np.meshgrid(k, k, indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), 0.1 * np.sin(3.0 * x.ravel()) * np.cos(2.0 * y.ravel())], 1)
    f = []
    for i in range(3):
        for j in range(3):
            a, b, c, d = 4 * i + j, 4 * (i + 1) + j, 4 * (i + 1) + j + 1, 4 * i + j + 1
            f += [(a, b, c), (a, c, d)]
    v = np.concatenate([v, [[2.0, 2.0, 2.0]], [0.5 * (v[0] + v[5])]])
    f += [(0, 17, 17), (5, 17, 5), (3, 3, 7)]                # repeated vertices: exactly zero normals
    v = np.concatenate([v, [v[10].copy()]])                  # vertex 18 = a copy of vertex 10
    f += [(10, 18, 6)]                                       # zero area: two corners at the same place
    return v, np.array(f, np.int64)


# ---- the noisy meshes of the property tests (fixed seeds) and their error measures ---------------------------------------
def noisy_sphere(seed=5, sigma=0.01):
    """meshray_ref.icosphere(3) with radial noise of `sigma` -> (verts, faces)"""
    import meshray_ref
    v, f = meshray_ref.icosphere(3)
    rng = np.random.default_rng(seed)
    return v * (1.0 + sigma * rng.standard_normal(len(v)))[:, None], f


def radial_stats(v):
    """(RMS of |v| - 1, mean |v|)"""
    r = np.linalg.norm(np.asarray(v, np.float64), axis=1)
    return float(np.sqrt(np.mean((r - 1.0) ** 2))), float(r.mean())


def noisy_cube(seed=11, sigma=0.02):
    """cube_mesh(8) with isotropic noise of `sigma` -> (verts, faces, side normals)"""
    v, f, side = cube_mesh(8)
    rng = np.random.default_rng(seed)
    return v + sigma * rng.standard_normal(v.shape), f, side


def mean_normal_angle(normals, side):
    """mean angle in degrees between the rows of `normals` and of `side`"""
    n = np.asarray(normals, np.float64)
    c = np.clip(np.abs((n * side).sum(1)) / np.maximum(np.linalg.norm(n, axis=1), 1e-300), 0.0, 1.0)
    return float(np.degrees(np.arccos(c)).mean())


def noisy_sheet(seed=5, sigma=0.01, n=12):
    """meshray_ref.grid_sheet(n), flat, with height noise of `sigma` -> (verts, faces, interior [V] bool)"""
    import meshray_ref
    v, f = meshray_ref.grid_sheet(n)
    v = np.array(v, np.float64)
    rng = np.random.default_rng(seed)
    v[:, 2] = sigma * rng.standard_normal(len(v))
    return v, np.asarray(f, np.int64), ~border_vertices(f, len(v))
