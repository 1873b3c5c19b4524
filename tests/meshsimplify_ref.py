"""numpy restatement of the mesh simplification (neuraludf_amd/meshclean.py simplify_mesh / simplify_to_faces,
csrc/meshsimplify.hip), for the tests: vertex clustering on a uniform grid (Rossignac-Borrel), each cluster's
representative placed by quadric error minimisation (Lindstrom) with boundary quadrics, a regularised 3 x 3 Cholesky solve
and an accept-inside-the-cell test.  float64 throughout, every product, sum, quotient and square root a separate
correctly rounded operation in the order the kernel takes them; the sums over a cluster's corners and members run in list
order (vectorised over the clusters, sequential inside each).  Plus the test inputs.  A plain helper module, not a
conftest."""
from typing import NamedTuple

import numpy as np

MAX_GRID = 1 << 20
BISECT_ROUNDS = 24


class Simplified(NamedTuple):
    """the public result's six fields, then what the tests look at besides: quadric [V', 10] (A00 A01 A02 A11 A12 A22 b0 b1
    b2 c of every output vertex's cluster), grid [3], clusters (before the unreferenced ones are dropped) and wall_margin
    (the smallest distance, in cells, of any cluster's quadric solution from a wall of its cell; inf without solutions)"""
    verts: np.ndarray
    faces: np.ndarray
    vertex_cluster: np.ndarray
    face_src: np.ndarray
    accepted: np.ndarray
    attributes: object
    quadric: np.ndarray
    grid: np.ndarray
    clusters: int
    wall_margin: float


# ---- rule 1: keys ------------------------------------------------------------------------------------------------------
def bounding_origin(verts):
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3).min(0)


def grid_dims(verts, origin, cell):
    """G = max c + 1 per axis; floor((p - origin) / cell) is monotone in p, so the maximum is that of the largest p"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex")
    g = np.floor((v.max(0) - origin) / cell) + 1.0
    if (v.min(0) < origin).any():
        raise ValueError("origin above the bounding box's minimum")
    if (g > MAX_GRID).any():
        raise ValueError("grid dimension above 2^20")
    return g.astype(np.int64)


def keys_of(p, origin, cell, grid):
    """key = (cx Gy + cy) Gz + cz in int64 with c = floor((p - origin) / cell); -1 for a point that is not finite or lies
    outside the grid"""
    with np.errstate(invalid="ignore"):
        c = np.floor((np.asarray(p, dtype=np.float64) - origin) / cell)
        ok = (np.isfinite(c) & (c >= 0) & (c < grid)).all(-1)
    ci = np.where(ok[..., None], c, 0.0).astype(np.int64)
    key = (ci[..., 0] * grid[1] + ci[..., 1]) * grid[2] + ci[..., 2]
    return np.where(ok, key, -1)


def cell_centres(key, origin, cell, grid):
    c = np.stack([key // (grid[1] * grid[2]), key // grid[2] % grid[1], key % grid[2]], -1).astype(np.float64)
    return origin + (c + 0.5) * cell


# ---- rule 2: clusters --------------------------------------------------------------------------------------------------
def _csr(group, n_groups):
    """items grouped by `group`, ascending inside each (stable sort) -> (offsets [n_groups + 1], items)"""
    items = np.argsort(group, kind="stable")
    off = np.zeros(n_groups + 1, dtype=np.int64)
    np.cumsum(np.bincount(group, minlength=n_groups), out=off[1:])
    return off, items


def _sequential_sum(off, terms):
    """per group g the sum of terms[off[g] : off[g + 1]] (rows of any width) added one after the other in list order"""
    n = len(off) - 1
    count = off[1:] - off[:-1]
    acc = np.zeros((n,) + terms.shape[1:], dtype=np.float64)
    for r in range(int(count.max()) if n else 0):
        g = np.nonzero(count > r)[0]
        acc[g] = acc[g] + terms[off[g] + r]
    return acc


# ---- rule 3: quadrics --------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _length(a):
    return np.sqrt(_dot(a, a))


def _plane_terms(u, through, centre, w, valid):
    """the ten numbers (w u u^T, w d u, w d^2) of the plane with unit normal u through `through`, local to `centre`;
    zeros where not valid"""
    with np.errstate(all="ignore"):
        d = -_dot(u, through - centre)
        wd = w * d
        cols = [w * (u[:, i] * u[:, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        cols += [wd * u[:, 0], wd * u[:, 1], wd * u[:, 2], wd * d]
    return np.where(valid[:, None], np.stack(cols, -1), 0.0)


def boundary_half_edges(faces, n_verts):
    """[3 F] bool: half-edge 3 f + k (faces[f][k] -> faces[f][(k + 1) % 3]) lies on an undirected edge with one half-edge"""
    a, b = faces.reshape(-1), np.roll(faces, -1, 1).reshape(-1)
    key = np.minimum(a, b) * n_verts + np.maximum(a, b)
    _, inverse, count = np.unique(key, return_inverse=True, return_counts=True)
    return count[inverse] == 1


def cluster_quadrics(v, faces, corner_off, corner, centre, boundary_weight):
    """[C, 10]: per cluster the sum over its corners (ascending 3 f + k) of the face plane, then the boundary plane of the
    half-edge that starts at the corner, then that of the half-edge that ends there"""
    f, k = corner // 3, corner % 3
    ctr = np.repeat(centre, corner_off[1:] - corner_off[:-1], axis=0)          # the centre of each listed corner's cluster
    p = v[faces[f]]                                                           # [n, 3 corners, 3]
    with np.errstate(all="ignore"):
        n = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        length = _length(n)
        face_ok = (length > 0) & np.isfinite(length)
        u = n / length[:, None]
        w = length * 0.5
    terms = np.zeros((len(corner), 3, 10), dtype=np.float64)
    terms[:, 0] = _plane_terms(u, p[:, 0], ctr, w, face_ok)
    if boundary_weight != 0:
        on_border = boundary_half_edges(faces, len(v))
        rows = np.arange(len(corner))
        for slot, j in ((1, k), (2, (k + 2) % 3)):                            # the half-edge from / into the corner
            start, end = p[rows, j], p[rows, (j + 1) % 3]
            with np.errstate(all="ignore"):
                m = _cross(end - start, u)
                mlen = _length(m)
                ok = face_ok & on_border[3 * f + j] & (mlen > 0) & np.isfinite(mlen)
                terms[:, slot] = _plane_terms(m / mlen[:, None], start, ctr, boundary_weight * w, ok)
    return _sequential_sum(3 * corner_off, terms.reshape(-1, 10))


# ---- rule 4: placement -------------------------------------------------------------------------------------------------
def solve(q, mean, lam):
    """x of (A + lam t I) x = -b + lam t mean, t = tr A, by Cholesky without pivoting -> (x [C, 3], t [C])"""
    with np.errstate(all="ignore"):
        t = (q[:, 0] + q[:, 3]) + q[:, 5]
        lt = lam * t
        m00, m10, m20, m11, m21, m22 = q[:, 0] + lt, q[:, 1], q[:, 2], q[:, 3] + lt, q[:, 4], q[:, 5] + lt
        r0, r1, r2 = -q[:, 6] + lt * mean[:, 0], -q[:, 7] + lt * mean[:, 1], -q[:, 8] + lt * mean[:, 2]
        l00 = np.sqrt(m00)
        l10, l20 = m10 / l00, m20 / l00
        l11 = np.sqrt(m11 - l10 * l10)
        l21 = (m21 - l20 * l10) / l11
        l22 = np.sqrt((m22 - l20 * l20) - l21 * l21)
        y0 = r0 / l00
        y1 = (r1 - l10 * y0) / l11
        y2 = ((r2 - l20 * y0) - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = ((y0 - l10 * x1) - l20 * x2) / l00
    return np.stack([x0, x1, x2], -1), t


# ---- rule 5: faces -----------------------------------------------------------------------------------------------------
def surviving_faces(faces, vcluster):
    """-> (remapped faces of the survivors, their source indices ascending): no repeated id, and of the faces with the
    same three ids the one with the smallest source index"""
    r = vcluster[faces]
    src = np.nonzero((r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2]))[0]
    t = np.sort(r[src], 1)
    order = np.lexsort((src, t[:, 2], t[:, 1], t[:, 0]))
    ts = t[order]
    first = np.ones(len(order), dtype=bool)
    first[1:] = (ts[1:] != ts[:-1]).any(1)
    keep = np.sort(src[order[first]])
    return r[keep], keep


def _clusters(v, origin, cell, grid):
    key = keys_of(v, origin, cell, grid)
    if (key < 0).any():
        raise ValueError("non-finite vertex")
    cluster_key, vcluster = np.unique(key, return_inverse=True)
    return cluster_key, vcluster.reshape(-1).astype(np.int64)


def count_faces(verts, faces, cell, origin=None):
    """rule 7's count-only pass: keys, unique, remap, dedupe -> F'"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    origin = bounding_origin(v) if origin is None else np.asarray(origin, dtype=np.float64)
    _, vcluster = _clusters(v, origin, cell, grid_dims(v, origin, cell))
    return len(surviving_faces(np.asarray(faces, dtype=np.int64), vcluster)[1])


def simplify(verts, faces, cell, origin=None, boundary_weight=1.0, regularisation=1e-3, placement="quadric",
             attributes=None):
    dtype = np.asarray(verts).dtype
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    attrs = None if attributes is None else np.asarray(attributes)
    if len(v) == 0 or len(faces) == 0:
        return Simplified(np.zeros((0, 3), dtype), np.zeros((0, 3), np.int64), np.full(len(v), -1, np.int64),
                          np.zeros(0, np.int64), np.zeros(0, bool), None if attrs is None else attrs[:0],
                          np.zeros((0, 10)), np.zeros(3, np.int64), 0, np.inf)
    cell = float(cell)
    origin = bounding_origin(v) if origin is None else np.asarray(origin, dtype=np.float64)
    grid = grid_dims(v, origin, cell)
    cluster_key, vcluster = _clusters(v, origin, cell, grid)
    n_clusters = len(cluster_key)
    centre = cell_centres(cluster_key, origin, cell, grid)
    member_off, member = _csr(vcluster, n_clusters)
    count = (member_off[1:] - member_off[:-1]).astype(np.float64)
    mean = _sequential_sum(member_off, v[member] - centre[vcluster[member]]) / count[:, None]
    quadric = np.zeros((n_clusters, 10))
    accepted = np.zeros(n_clusters, dtype=bool)
    rep, margin = mean, np.inf
    if placement == "quadric":
        corner_off, corner = _csr(vcluster[faces.reshape(-1)], n_clusters)
        quadric = cluster_quadrics(v, faces, corner_off, corner, centre, float(boundary_weight))
        x, t = solve(quadric, mean, float(regularisation))
        with np.errstate(invalid="ignore"):
            accepted = (t > 0) & (keys_of(centre + x, origin, cell, grid) == cluster_key)
            solved = (t > 0) & np.isfinite(x).all(1)
            if solved.any():
                margin = float(np.abs(np.abs(x[solved]) - 0.5 * cell).min() / cell)
        rep = np.where(accepted[:, None], x, mean)
    elif placement != "mean":
        raise ValueError(placement)
    pos = centre + rep
    new_faces, face_src = surviving_faces(faces, vcluster)
    kept = np.zeros(n_clusters, dtype=bool)
    kept[new_faces.reshape(-1)] = True
    remap = np.where(kept, np.cumsum(kept) - 1, -1)
    out_attr = None
    if attrs is not None:
        a = attrs.astype(np.float64).reshape(len(v), -1)
        out_attr = (_sequential_sum(member_off, a[member]) / count[:, None])[kept].astype(attrs.dtype)
    return Simplified(pos[kept].astype(dtype), remap[new_faces], remap[vcluster], face_src, accepted[kept], out_attr,
                      quadric[kept], grid, n_clusters, margin)


# ---- rule 7 ------------------------------------------------------------------------------------------------------------
def bisect_cell(side, n):
    """the cell for n cells along a side: a hair above side / n, so that the largest vertex falls into cell n - 1 and not
    into a cell n of its own"""
    return side / n * (1.0 + 1e-9)


def bisect_cells(verts, faces, target_faces):
    """-> (cells along the longest bounding-box side, cell): the largest count the bisection finds whose F' is at most
    target_faces; F' is not strictly monotone in the grid, so a finer grid that also fits may exist"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    side = float((v.max(0) - v.min(0)).max())
    side = side if side > 0 else 1.0
    lo, hi = 1, min(MAX_GRID - 1, max(1, len(v)))
    for _ in range(BISECT_ROUNDS):
        if lo >= hi:
            break
        mid = (lo + hi + 1) // 2
        if count_faces(v, faces, bisect_cell(side, mid)) <= target_faces:
            lo = mid
        else:
            hi = mid - 1
    return lo, bisect_cell(side, lo)


def simplify_to_faces(verts, faces, target_faces, **kw):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(faces) <= target_faces:
        return None                                           # the input comes back unchanged
    return simplify(verts, faces, bisect_cells(verts, faces, target_faces)[1], **kw)


# ---- inputs ------------------------------------------------------------------------------------------------------------
SHEET_LO, SHEET_HI, SHEET_QUADS = -0.83, 0.79, 48
FOLD_X, FOLD_DEG, FOLD_ROT = 0.037, 70.0, 0.3


def lowered_origin(verts, cell, fraction=0.185):
    """the bounding-box minimum lowered by a fraction of a cell: a flat part of the mesh at the minimum then lies inside
    the first layer of cells, not on its wall, where the accept test would hang on the last bit"""
    return bounding_origin(verts) - fraction * cell


def sheet(n=SHEET_QUADS, lo=SHEET_LO, hi=SHEET_HI):
    """n x n quads (two triangles each, wound alike) over [lo, hi]^2 in the plane z = 0 -> (verts float64, faces int64)"""
    ax = np.linspace(lo, hi, n + 1)
    x, y = np.meshgrid(ax, ax, indexing="ij")
    verts = np.stack([x.reshape(-1), y.reshape(-1), np.zeros((n + 1) ** 2)], -1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    b, c, d = a + (n + 1), a + (n + 2), a + 1
    return verts, np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)]).astype(np.int64)


def fold_frame():
    """(point on the crease, unit direction of the crease, unit normals of the two half-planes) of folded_sheet()"""
    th, rot = np.radians(FOLD_DEG), FOLD_ROT
    R = np.array([[np.cos(rot), -np.sin(rot), 0.0], [np.sin(rot), np.cos(rot), 0.0], [0.0, 0.0, 1.0]])
    return (R @ np.array([FOLD_X, 0.0, 0.0]), R @ np.array([0.0, 1.0, 0.0]), R @ np.array([0.0, 0.0, 1.0]),
            R @ np.array([-np.sin(th), 0.0, np.cos(th)]))


def folded_sheet():
    """the sheet folded by FOLD_DEG along x = FOLD_X (the part beyond the line turns up about it), then rotated by
    FOLD_ROT about z"""
    v, f = sheet()
    th, rot = np.radians(FOLD_DEG), FOLD_ROT
    s = np.maximum(v[:, 0] - FOLD_X, 0.0)
    v = np.stack([np.minimum(v[:, 0], FOLD_X) + s * np.cos(th), v[:, 1], s * np.sin(th)], -1)
    R = np.array([[np.cos(rot), -np.sin(rot), 0.0], [np.sin(rot), np.cos(rot), 0.0], [0.0, 0.0, 1.0]])
    return v @ R.T, f


def sphere_mesh(n=24, radius=0.6):
    """the marching-cubes sphere of tests/meshudf_ref.py at resolution n -> (verts float64, faces int64)"""
    import meshudf_ref as R
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    U, G, axes = R.sphere_grid(n, radius)
    v, f = R.marching_cubes(U, G, axes, *box)
    return np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)


def dense_fan(segments=300, seed=5):
    """a fan of `segments` thin triangles around one hub vertex with the rim in the cells around the hub's (unit grid): the
    hub's cluster holds `segments` corners, the rim's clusters several dozen each; next to it a bumpy 8 x 8 sheet over
    ordinary cells -> (verts, faces, cell)"""
    v, f = sheet(8, 0.0, 4.0)
    rng = np.random.default_rng(seed)
    v[:, 2] = 0.3 * rng.random(len(v))
    ang = np.linspace(0.0, 2.0 * np.pi, segments, endpoint=False)
    hub = np.array([[6.47, 1.53, 0.41]])
    rim = hub + np.stack([1.21 * np.cos(ang), 1.17 * np.sin(ang), 0.1 * np.sin(3.0 * ang)], -1)
    i = np.arange(segments)
    fan = np.stack([np.zeros(segments, dtype=np.int64), 1 + i, 1 + (i + 1) % segments], -1) + len(v)
    return np.concatenate([v, hub, rim]), np.concatenate([f, fan]).astype(np.int64), 1.0


def disc_mesh(n=32, rho=0.5, c=0.0123):
    """the marching-cubes mesh of a flat disc of radius rho at z = c (an open surface with one border loop)"""
    import meshudf_ref as R
    import torch
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    axes = np.stack([torch.linspace(-1.0, 1.0, n).numpy() for _ in range(3)])
    p = np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(np.float64)
    s = np.linalg.norm(p[..., :2], axis=-1, keepdims=True)
    dz = p[..., 2:3] - c
    out = np.maximum(s - rho, 0.0)
    u = np.sqrt(out * out + dz * dz)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.nan_to_num(np.concatenate([out * np.nan_to_num(p[..., :2] / s), dz], -1) / u)
    v, f = R.marching_cubes(u[..., 0].astype(np.float32), g.astype(np.float32), axes.astype(np.float32), *box)
    keep = np.linalg.norm(v[:, :2], axis=1) < rho + 2.0 / (n - 1)              # filter_mesh's job: drop the far rim
    keep = keep[f].all(1)
    return np.asarray(v, dtype=np.float64), np.asarray(f[keep], dtype=np.int64)


def key_patch(cell=0.37, seed=9):
    """a bumpy 10 x 10-quad patch (200 faces) over a few cells and an origin so far below it that every grid dimension is
    2^20 - 1 and the keys lie between 2^59 and 2^60: any int32 or float32 step in the key path shows
    -> (verts, faces, cell, origin)"""
    v, f = sheet(10, 0.0, 2.1)
    rng = np.random.default_rng(seed)
    v = v + np.array([0.0, 0.0, 0.9]) * rng.random((len(v), 1)) + 0.05 * rng.random((len(v), 3))
    origin = v.max(0) - (MAX_GRID - 2 + 0.37) * cell
    return v, f, cell, origin


_CASES = {}


def cases():
    """the inputs of the GPU comparison, built once: name -> dict(v, f, cell, origin, attributes); read-only arrays"""
    if not _CASES:
        import meshorient_ref as O
        rng = np.random.default_rng(3)
        fold_v, fold_f = folded_sheet()
        flat_v, flat_f = sheet()
        sph_v, sph_f = sphere_mesh()
        mix_v, mix_f = O.mixed_mesh((sph_v, sph_f), disc_mesh())
        fan_v, fan_f, fan_cell = dense_fan()
        for name, v, f, cell, lowered in (("fold", fold_v, fold_f, 0.17, True), ("flat", flat_v, flat_f, 0.11, True),
                                          ("sphere", sph_v, sph_f, 0.2, False), ("mixed", mix_v, mix_f, 0.23, True),
                                          ("fan", fan_v, fan_f, fan_cell, True)):
            case = dict(v=v, f=f, cell=cell, origin=lowered_origin(v, cell) if lowered else None,
                        attributes=rng.random((len(v), 3)))
            for a in case.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _CASES[name] = case
    return _CASES
