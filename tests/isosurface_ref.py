"""numpy restatement of the level-set mesher (neuraludf_amd/meshing.py iso_*, csrc/isosurface.hip) over the library's
generated case table, for the tests: the cell rule (corner `-` iff F < level in fp32; a non-finite corner silences the
cell), the edge rule (t = (level - F_a) / (F_b - F_a), every operation rounded to fp32, clamped to [0, 1], 0.5 if NaN),
the ordering (vertices by edge id, faces by cell and table order) and the block selection of the sparse path; plus the
analytic fields and the table-backed stand-in the CPU and GPU tests share.  Loops over the cut cells in Python: keep
N <= 64.  A plain helper module, not a conftest."""
import numpy as np
import torch

from neuraludf_amd import mc_tables as T

TRI = T.tables()
NTRI = np.array([len(t) for t in TRI], dtype=np.int64)
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
NONCUBIC = ((-0.8, -0.7, -0.5), (0.9, 0.75, 0.6))


def grid_axes(n, bound_min, bound_max):
    """[3, n] fp32: the library's grid coordinates (torch.linspace per axis)"""
    return np.stack([torch.linspace(float(bound_min[a]), float(bound_max[a]), n).numpy() for a in range(3)])


def cell_cases(F, level):
    """-> (case [m, m, m], ntri [m, m, m]) of every cell; case 0 where a corner is NaN or infinite"""
    F = np.asarray(F, dtype=np.float32)
    level = np.float32(level)
    m = F.shape[0] - 1
    case = np.zeros((m, m, m), dtype=np.int64)
    finite = np.ones((m, m, m), dtype=bool)
    for c, (dx, dy, dz) in enumerate(T.CORNERS):
        v = F[dx:dx + m, dy:dy + m, dz:dz + m]
        with np.errstate(invalid="ignore"):
            case |= (v < level).astype(np.int64) << c
        finite &= np.isfinite(v)
    case[~finite] = 0
    return case, NTRI[case]


def marching_cubes(F, level, axes):
    """F [N, N, N] fp32, axes [3, N] fp32 (the grid coordinates) -> (verts [V, 3] fp32, faces [F, 3] int64)"""
    F = np.asarray(F, dtype=np.float32)
    axes = np.asarray(axes, dtype=np.float32)
    level = np.float32(level)
    n = F.shape[0]
    case, ntri = cell_cases(F, level)
    face_edges = []
    for i, j, k in np.argwhere(ntri > 0):                # C order = ascending cell index
        for tri in TRI[case[i, j, k]]:
            ids = []
            for e in tri:
                dx, dy, dz = T.CORNERS[T.EDGES[e][0]]
                ids.append(3 * (((i + dx) * n + j + dy) * n + k + dz) + T.EDGE_AXIS[e])
            face_edges.append(ids)
    face_edges = np.asarray(face_edges, dtype=np.int64).reshape(-1, 3)
    edges, faces = np.unique(face_edges, return_inverse=True)
    faces = faces.reshape(-1, 3).astype(np.int64)
    verts = np.empty((len(edges), 3), dtype=np.float32)
    for v, eid in enumerate(edges):
        p, axis = divmod(int(eid), 3)
        idx = [p // (n * n), (p // n) % n, p % n]
        hi = list(idx)
        hi[axis] += 1
        fa, fb = F[tuple(idx)], F[tuple(hi)]
        with np.errstate(all="ignore"):
            t = np.float32(np.float32(level - fa) / np.float32(fb - fa))
        t = np.float32(0.5) if np.isnan(t) else min(max(t, np.float32(0)), np.float32(1))
        for x in range(3):
            xa = axes[x, idx[x]]
            verts[v, x] = np.float32(xa + np.float32(t * np.float32(axes[x, idx[x] + 1] - xa))) if x == axis else xa
    return verts, faces


# ---- the sparse path's host side ----------------------------------------------------------------------------------------

def block_geometry(n, b):
    """-> (nb, coarse [nb + 1]): blocks per axis and the grid index min(t b, n - 1) of each coarse node"""
    nb = (n - 1 + b - 1) // b
    return nb, np.minimum(np.arange(nb + 1, dtype=np.int64) * b, n - 1)


def selection_bounds(bound_min, bound_max, n, level, b, lipschitz):
    """(lo, hi) fp32: level + lipschitz r rounded up and level - lipschitz r rounded down, from float64; level is the
    fp32 value the kernels compare with"""
    ha = np.array([(np.float64(bound_max[a]) - np.float64(bound_min[a])) / (n - 1) for a in range(3)])
    reach = np.float64(lipschitz) * (0.5 * np.sqrt(((b * ha) ** 2).sum()))
    lv = np.float64(np.float32(level))
    lo, hi = np.float32(lv + reach), np.float32(lv - reach)
    if np.float64(lo) < lv + reach:
        lo = np.nextafter(lo, np.float32(np.inf))
    if np.float64(hi) > lv - reach:
        hi = np.nextafter(hi, np.float32(-np.inf))
    assert np.float64(lo) >= lv + reach > np.float64(np.nextafter(lo, np.float32(-np.inf)))
    assert np.float64(hi) <= lv - reach < np.float64(np.nextafter(hi, np.float32(np.inf)))
    return lo, hi


def select(coarse, n, b, lo, hi):
    """ascending linear ids of the selected blocks; coarse: [(nb+1)^3] values at the coarse nodes.  A block with a NaN
    corner is not selected."""
    nb = block_geometry(n, b)[0]
    c = np.asarray(coarse, dtype=np.float32).reshape(nb + 1, nb + 1, nb + 1)
    out = []
    for bi in range(nb):
        for bj in range(nb):
            for bk in range(nb):
                v = c[bi:bi + 2, bj:bj + 2, bk:bk + 2]
                if not np.isnan(v).any() and v.min() <= lo and v.max() >= hi:
                    out.append((bi * nb + bj) * nb + bk)
    return np.asarray(out, dtype=np.int64)


def uncovered_cut_cells(F, level, blocks, b):
    """number of cells of the dense grid F with triangles that lie in no selected block"""
    n = F.shape[0]
    nb = block_geometry(n, b)[0]
    ijk = np.argwhere(cell_cases(F, level)[1] > 0)
    assert len(ijk) > 0
    return int((~np.isin(((ijk[:, 0] // b) * nb + ijk[:, 1] // b) * nb + ijk[:, 2] // b, blocks)).sum())


# ---- mesh properties ----------------------------------------------------------------------------------------------------

def directed_edges_unique(faces):
    """no directed edge (a -> b in a face's winding) appears twice: the mesh is consistently wound"""
    f = np.asarray(faces)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return len(np.unique(e, axis=0)) == len(e)


def signed_volume(verts, faces):
    """positive when the normals point away from the enclosed region"""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- fields (elementwise torch, fp32; pts [P, 3] -> [P]) ----------------------------------------------------------------

def _norm(*x):
    """sqrt of a sum of squares, one elementwise op at a time: the same bits whatever the batch"""
    s = x[0] * x[0]
    for y in x[1:]:
        s = s + y * y
    return torch.sqrt(s)


def sphere_sdf(p, radius=0.6):
    return _norm(p[..., 0], p[..., 1], p[..., 2]) - radius


def shell_udf(p, radius=0.6):
    return sphere_sdf(p, radius).abs()


def slab_sdf(p, rho=0.45, c=0.0371, half=0.08):
    """signed field of the slab-disc x^2 + y^2 <= rho^2, |z - c| <= half (negative inside, slope <= 1)"""
    return torch.maximum(_norm(p[..., 0], p[..., 1]) - rho, (p[..., 2] - c).abs() - half)


def plane_udf(p):
    return p[..., 2].abs()


def grid_values(fn, n, bound_min, bound_max, device="cpu"):
    """fp32 F [n, n, n] of a field on the dense grid (axes as the library's: torch.linspace per axis)"""
    ax = [torch.linspace(float(bound_min[a]), float(bound_max[a]), n, device=device) for a in range(3)]
    p = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return fn(p).float().reshape(n, n, n)


def coarse_values(fn, n, b, bound_min, bound_max):
    """the field at the coarse nodes, numpy [(nb+1)^3]"""
    idx = torch.from_numpy(block_geometry(n, b)[1])
    ax = [torch.linspace(float(bound_min[a]), float(bound_max[a]), n)[idx] for a in range(3)]
    p = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return fn(p).float().reshape(-1).numpy()


def random_field(n, seed, raise_boundary=False):
    """uniform [0, 1) fp32 [n, n, n]; raise_boundary: the boundary nodes are 2 (above any level in (0, 1))"""
    F = torch.rand((n, n, n), generator=torch.Generator().manual_seed(seed))
    if raise_boundary:
        F[0], F[-1], F[:, 0], F[:, -1], F[:, :, 0], F[:, :, -1] = 2.0, 2.0, 2.0, 2.0, 2.0, 2.0
    return F


SPECIAL_NODES = (((5, 7, 9), float("nan")), ((11, 3, 14), float("inf")), ((17, 18, 2), float("-inf")),
                 ((6, 6, 6), float("nan")), ((6, 6, 7), float("inf")), ((13, 21, 10), None), ((2, 15, 19), None),
                 ((19, 9, 13), None))          # none of them a coarse node of B = 4 or 8 at N = 24 (an index 0, 4, ..., 23)


def random_field_with_specials(n=24, seed=11, level=0.5):
    """the random field with a handful of nodes set to NaN, +inf, -inf and (None) exactly the level"""
    F = random_field(n, seed)
    for idx, val in SPECIAL_NODES:
        F[idx] = float(np.float32(level)) if val is None else val
    return F


class TableQuery:
    """query_func stand-in that returns the values of a grid volume F [N, N, N] at points that are grid nodes"""

    def __init__(self, F, bound_min, bound_max):
        from neuraludf_amd.models import udf_renderer_blending as rb
        self.F, self.n = F, F.shape[0]
        self.axes = rb._grid_axes(bound_min, bound_max, self.n, F.device)

    def __call__(self, pts):
        idx = [torch.searchsorted(self.axes[a], pts[:, a].contiguous()).clamp_max(self.n - 1) for a in range(3)]
        assert all(bool((self.axes[a][idx[a]] == pts[:, a]).all()) for a in range(3)), "a query point is no grid node"
        return self.F.reshape(-1)[(idx[0] * self.n + idx[1]) * self.n + idx[2]]
