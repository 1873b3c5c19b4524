"""numpy restatement of the sparse UDF extraction's host side (neuraludf_amd/meshing.py udf_sparse_grid): the block
geometry for exact and ragged N, the selection threshold (float64, rounded up to fp32), the selection, the set of grid
nodes of the selected blocks, the canonical ordering keys and the dense active-cell test; plus the analytic stand-in
fields the CPU and GPU tests share.  A plain helper module, not a conftest."""
import numpy as np
import torch

from neuraludf_amd.meshing import MAX_RATIO, grid_spacing, thresholds

NONCUBIC = ((-1.0, -0.8, -0.5), (1.0, 0.9, 0.6))
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def block_geometry(n, b):
    """-> (nb, lo [nb], hi [nb]): blocks per axis and the coarse node indices min(t b, n-1), min((t+1) b, n-1) of block
    t, which covers the cells [t b, min((t+1) b, n-1))"""
    m = n - 1
    nb = (m + b - 1) // b
    t = np.arange(nb, dtype=np.int64)
    return nb, np.minimum(t * b, n - 1), np.minimum((t + 1) * b, n - 1)


def threshold(bound_min, bound_max, n, b, lipschitz):
    """1.74 h + lipschitz r in float64, rounded up to fp32"""
    ha = np.array([(np.float64(bound_max[a]) - np.float64(bound_min[a])) / (n - 1) for a in range(3)])
    r = 0.5 * np.sqrt(((b * ha) ** 2).sum())
    t = np.float64(MAX_RATIO) * ha.max() + np.float64(lipschitz) * r
    f = np.float32(t)
    if np.float64(f) < t:
        f = np.nextafter(f, np.float32(np.inf))
    assert np.float64(f) >= t and np.float64(np.nextafter(f, np.float32(-np.inf))) < t
    return f


def coarse_indices(n, b):
    """grid index of each of the nb+1 coarse nodes per axis"""
    nb = block_geometry(n, b)[0]
    return np.minimum(np.arange(nb + 1, dtype=np.int64) * b, n - 1)


def select(coarse, n, b, thr):
    """ascending linear ids of the selected blocks; coarse: [nb+1, nb+1, nb+1] values at the coarse nodes"""
    nb = block_geometry(n, b)[0]
    c = np.asarray(coarse, dtype=np.float32).reshape(nb + 1, nb + 1, nb + 1)
    c = np.where(np.isnan(c), np.float32(np.inf), np.maximum(c, np.float32(0)))
    out = []
    for bi in range(nb):
        for bj in range(nb):
            for bk in range(nb):
                if c[bi:bi + 2, bj:bj + 2, bk:bk + 2].min() <= thr:
                    out.append((bi * nb + bj) * nb + bk)
    return np.asarray(out, dtype=np.int64)


def node_mask(blocks, n, b):
    """[n, n, n] bool: the grid nodes that belong to at least one of `blocks`"""
    nb, lo, hi = block_geometry(n, b)
    mask = np.zeros((n, n, n), dtype=bool)
    for blk in np.asarray(blocks).tolist():
        bi, bj, bk = blk // (nb * nb), (blk // nb) % nb, blk % nb
        mask[lo[bi]:hi[bi] + 1, lo[bj]:hi[bj] + 1, lo[bk]:hi[bk] + 1] = True
    return mask


def unique_nodes(blocks, n, b):
    """ascending linear ids (i n + j) n + k of those nodes"""
    return np.flatnonzero(node_mask(blocks, n, b).reshape(-1)).astype(np.int64)


def cell_key(i, j, k, n):
    """faces are ordered by this key of their cell, then by table order"""
    return (np.asarray(i, dtype=np.int64) * (n - 1) + j) * (n - 1) + k


def edge_key(i, j, k, axis, n):
    """vertices are ordered by this key of their edge: 3 lin(lower end) + axis"""
    return 3 * ((np.asarray(i, dtype=np.int64) * n + j) * n + k) + axis


def block_of_cell(i, j, k, n, b):
    nb = block_geometry(n, b)[0]
    return ((np.asarray(i, dtype=np.int64) // b) * nb + np.asarray(j) // b) * nb + np.asarray(k) // b


def active_cells(U, bound_min, bound_max):
    """[n-1, n-1, n-1] bool: the dense mesher's active test on an fp32 grid (as meshudf_ref.marching_cubes)"""
    U = np.asarray(U, dtype=np.float32)
    n = U.shape[0]
    m = n - 1
    mean_thr, max_thr = thresholds(grid_spacing(bound_min, bound_max, n))
    corner = [U[dx:dx + m, dy:dy + m, dz:dz + m] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    s = corner[0].copy()
    for c in range(1, 8):
        s = (s + corner[c]).astype(np.float32)
    return (s * np.float32(0.125) < mean_thr) & (np.max(np.stack(corner), 0) <= max_thr)


def uncovered_active_cells(U, blocks, b, bound_min, bound_max):
    """number of active cells of the dense grid U that lie in no selected block"""
    n = U.shape[0]
    ijk = np.argwhere(active_cells(U, bound_min, bound_max))
    assert len(ijk) > 0
    return int((~np.isin(block_of_cell(ijk[:, 0], ijk[:, 1], ijk[:, 2], n, b), blocks)).sum())


# ---- analytic stand-ins (elementwise torch, fp32; the formulas of tests/test_gpu_meshudf.py) -------------------------

def sphere_udf(p, radius=0.6):
    r = p.norm(dim=-1, keepdim=True)
    return (r - radius).abs(), torch.nan_to_num(p / r * torch.sign(r - radius))


def disc_udf(p, rho=0.5, c=0.0123):
    """distance to the disc x^2 + y^2 <= rho^2, z = c, and its gradient"""
    s = p[..., :2].norm(dim=-1, keepdim=True)
    dz = p[..., 2:3] - c
    out = (s - rho).clamp_min(0.0)
    u = torch.sqrt(out * out + dz * dz)
    return u, torch.nan_to_num(torch.cat([out * torch.nan_to_num(p[..., :2] / s), dz], -1) / u)


class Field(torch.nn.Module):
    """a stand-in for the UDF network: .udf(pts) -> [P, 1], .gradient(pts) -> [P, 1, 3] from fn(pts) -> (u [P, 1],
    g [P, 3]); one dummy parameter gives it a device.  Records the points of every udf() call."""

    def __init__(self, fn, record=False):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.fn, self.seen = fn, ([] if record else None)

    def udf(self, pts):
        if self.seen is not None:
            self.seen.append(pts.detach().clone())
        return self.fn(pts)[0].float()

    def gradient(self, pts):
        return self.fn(pts)[1].float()[:, None, :]


def grid_values(fn, n, bound_min, bound_max, device="cpu"):
    """fp32 U [n, n, n] of a stand-in on the dense grid (axes as the library's: torch.linspace per axis)"""
    ax = [torch.linspace(float(bound_min[a]), float(bound_max[a]), n, device=device) for a in range(3)]
    p = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return fn(p)[0].float().reshape(n, n, n)


def coarse_values(fn, n, b, bound_min, bound_max):
    """the stand-in at the coarse nodes, numpy [nb+1, nb+1, nb+1]"""
    idx = torch.from_numpy(coarse_indices(n, b))
    ax = [torch.linspace(float(bound_min[a]), float(bound_max[a]), n)[idx] for a in range(3)]
    p = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return fn(p)[0].float().reshape(len(idx), len(idx), len(idx)).numpy()
