"""GPU: sparse UDF extraction (neuraludf_amd/meshing.py udf_sparse_grid / udf_marching_cubes_sparse,
csrc/meshudf_sparse.hip) -- the sparse mesher against the dense one on the same values, order included; the selection,
the node list and the counters against the numpy restatement (tests/meshudf_sparse_ref.py); sparse against truly dense
extraction for distance fields; the network; a grid beyond the dense limit; pass-through and errors."""
import math

import numpy as np
import pytest
import torch

import meshudf_ref as R
import meshudf_sparse_ref as S
from common import build_modules, perturb_

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = S.BOX
LIP = 1.05       # the analytic stand-ins are true distance fields


class TableField(torch.nn.Module):
    """a stand-in that returns given grid volumes U [N, N, N], G [N, N, N, 3] at points that are grid nodes"""

    def __init__(self, U, G, bmin, bmax):
        super().__init__()
        from neuraludf_amd.models import udf_renderer_blending as rb
        self.dummy = torch.nn.Parameter(torch.zeros(1, device=U.device))
        self.U, self.G, self.n = U, G, U.shape[0]
        self.axes = rb._grid_axes(bmin, bmax, self.n, U.device)

    def _lin(self, pts):
        idx = [torch.searchsorted(self.axes[a], pts[:, a].contiguous()).clamp_max(self.n - 1) for a in range(3)]
        assert all(bool((self.axes[a][idx[a]] == pts[:, a]).all()) for a in range(3)), "a query point is no grid node"
        return (idx[0] * self.n + idx[1]) * self.n + idx[2]

    def udf(self, pts):
        return self.U.reshape(-1)[self._lin(pts)][:, None]

    def gradient(self, pts):
        return self.G.reshape(-1, 3)[self._lin(pts)][:, None, :]


def _analytic(fn):
    return S.Field(fn).to(DEV)


def _random_table(n, seed):
    from neuraludf_amd import meshing
    h = meshing.grid_spacing(*BOX, n)
    g = torch.Generator().manual_seed(seed)
    U = (torch.rand((n, n, n), generator=g) * (1.2 * h)).to(DEV)
    G = torch.randn((n, n, n, 3), generator=g).to(DEV)
    return TableField(U, G, *BOX)


@pytest.fixture(scope="module")
def network():
    from neuraludf_amd.models import fields
    return build_modules(fields, seed=0)["udf"].to(DEV)


@pytest.fixture(scope="module")
def network_dense(network):
    """the dense grid and raw dense mesh of the geometric-init network at N = 96 (computed once, left unchanged)"""
    from neuraludf_amd import meshing
    U, G = meshing.udf_grid(network, 96)
    v, f = meshing.udf_marching_cubes(U, G, *BOX)
    return U, G, v, f


def _exactness_case(name):
    """-> (stand-in, N, box, lipschitz)"""
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    if name == "sphere65":
        return _analytic(S.sphere_udf), 65, BOX, LIP
    if name == "sphere96":
        return _analytic(S.sphere_udf), 96, BOX, LIP
    if name == "disc96_noncubic":
        return _analytic(S.disc_udf), 96, S.NONCUBIC, LIP
    if name == "random24":
        return _random_table(24, 5), 24, BOX, 2.0
    if name == "random5":
        return _random_table(5, 6), 5, BOX, 2.0
    assert name == "network48"
    udf = perturb_(build_modules(fields, seed=0))["udf"].to(DEV)
    return TableField(*meshing.udf_grid(udf, 48), *BOX), 48, BOX, 2.0


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("name", ["sphere65", "sphere96", "disc96_noncubic", "random24", "random5", "network48"])
def test_sparse_mesher_equals_dense_mesher_on_the_same_values(name, b):
    """unconditional: whatever the field's slope, the sparse mesher gives the dense mesher's mesh of to_dense(), order
    included (N = 48 with B = 8: block faces; N = 5 with B = 8: one ragged block, padding)"""
    from neuraludf_amd import meshing
    field, n, (bmin, bmax), lip = _exactness_case(name)
    g = meshing.udf_sparse_grid(field, n, bmin, bmax, block=b, lipschitz=lip)
    v, f = meshing.udf_marching_cubes_sparse(g)
    dv, df = meshing.udf_marching_cubes(*g.to_dense(), bmin, bmax)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and f.shape[0] > 0
    print(f"{name} B={b}: {g.n_blocks} of {g.nb ** 3} blocks, {f.shape[0]} faces, {v.shape[0]} vertices")
    assert torch.equal(f, df)
    assert torch.equal(v, dv)
    assert int(f.min()) >= 0 and int(f.max()) == v.shape[0] - 1 and bool(torch.isfinite(v).all())


@pytest.mark.parametrize("b", [4, 8])
def test_selection_nodes_and_counters(b):
    from neuraludf_amd import meshing
    n = 96
    field = S.Field(S.sphere_udf, record=True).to(DEV)
    g = meshing.udf_sparse_grid(field, n, *BOX, block=b, lipschitz=LIP)
    nb = S.block_geometry(n, b)[0]
    assert (g.N, g.B, g.nb, g.n_coarse) == (n, b, nb, (nb + 1) ** 3) and g.coarse.shape == ((nb + 1) ** 3,)
    blocks = S.select(g.coarse.cpu().numpy(), n, b, S.threshold(*BOX, n, b, LIP))
    np.testing.assert_array_equal(g.blocks.cpu().numpy(), blocks)
    assert 0 < g.n_blocks == len(blocks) < nb ** 3
    nodes = S.unique_nodes(blocks, n, b)
    assert g.n_queried == len(nodes)
    slot = g.block_slot.cpu().numpy()
    assert slot.dtype == np.int32 and (slot[blocks] == np.arange(len(blocks))).all() and (slot >= 0).sum() == len(blocks)
    # the stand-in saw the coarse nodes, then every fine node exactly once, and only points that are grid nodes
    seen = torch.cat(field.seen)
    assert seen.shape[0] == g.n_coarse + g.n_queried
    lin = TableField(torch.zeros((n, n, n), device=DEV), torch.zeros((n, n, n, 3), device=DEV), *BOX)._lin
    ci = torch.from_numpy(S.coarse_indices(n, b)).to(DEV)
    coarse_lin = ((ci[:, None, None] * n + ci[None, :, None]) * n + ci[None, None, :]).reshape(-1)
    assert torch.equal(lin(seen[:g.n_coarse]), coarse_lin)
    np.testing.assert_array_equal(lin(seen[g.n_coarse:]).cpu().numpy(), nodes)
    # brick copies of a shared node are the same bits; the padding is +inf / 0
    ids = g.node_ids()
    Ud, Gd = g.to_dense()
    keep = ids >= 0
    assert torch.equal(g.U[keep].view(torch.int32), Ud.reshape(-1)[ids[keep]].view(torch.int32))
    assert torch.equal(g.G[keep].view(torch.int32), Gd.reshape(-1, 3)[ids[keep]].view(torch.int32))
    assert bool(torch.isinf(g.U[~keep]).all()) and not bool(g.G[~keep].any())
    h = meshing.grid_spacing(*BOX, n)
    assert g.n_grad == int((Ud < 2.0 * h).sum()) > 0
    assert int(torch.isinf(Ud).sum()) == n ** 3 - len(nodes)


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("n", [65, 96])
@pytest.mark.parametrize("fn", [S.sphere_udf, S.disc_udf], ids=["sphere", "disc"])
def test_sparse_equals_truly_dense_for_distance_fields(fn, n, b):
    from neuraludf_amd import meshing
    field = _analytic(fn)
    v, f = meshing.udf_marching_cubes_sparse(meshing.udf_sparse_grid(field, n, *BOX, block=b, lipschitz=LIP))
    dv, df = meshing.udf_marching_cubes(*meshing.udf_grid(field, n, *BOX), *BOX)
    assert f.shape[0] > 0 and torch.equal(f, df) and torch.equal(v, dv)
    for clean in (dict(), dict(fill_holes=True, smooth_borders=True, keep_largest=True)):
        sv, sf = meshing.extract_udf_mesh(field, n, sparse=True, block=b, lipschitz=LIP, **clean)
        ev, ef = meshing.extract_udf_mesh(field, n, **clean)
        assert sv.dtype == np.float32 and sf.dtype == np.int64 and len(sf) > 0
        assert sv.tobytes() == ev.tobytes() and sf.tobytes() == ef.tobytes()


def test_network(network, network_dense):
    """geometric-init UDFNetwork, N = 96, B = 8, default lipschitz.  Face-for-face equality with the truly dense network
    mesh is not asserted (gradient() runs a per-tile-scaled backward sweep: the last bits of G may depend on tile-mates
    and can flip a near-zero dot); the number of differing faces is printed."""
    from neuraludf_amd import meshing
    n, b = 96, 8
    U, G, dv, df = network_dense
    g = meshing.udf_sparse_grid(network, n)
    assert (g.B, g.nb) == (b, 12) and 0 < g.n_blocks < g.nb ** 3
    # (a) every brick value is the dense grid's value at that node, bit for bit
    ids = g.node_ids()
    keep = ids >= 0
    diff = g.U[keep].view(torch.int32) != U.reshape(-1)[ids[keep]].view(torch.int32)
    print(f"brick values that differ from the dense grid's: {int(diff.sum())} of {int(keep.sum())}")
    assert not bool(diff.any())
    # (b) every active cell of the dense U lies in a selected block
    assert S.uncovered_active_cells(U.cpu().numpy(), g.blocks.cpu().numpy(), b, *BOX) == 0
    # (c) the mesh: one component, the hole structure the dense test asserts
    v, f = meshing.extract_udf_mesh(network, n, sparse=True)
    assert v.dtype == np.float32 and f.dtype == np.int64
    _, cnt = R.edge_counts(f)
    n_boundary, holes = R.boundary_loops(len(v), f)
    assert cnt.max() == 2 and R.components(len(v), f) == 1
    assert R.euler(len(v), f) == 2 - holes and n_boundary == 3 * holes and holes <= 20, (n_boundary, holes)
    # (d) two runs are identical bytes
    v2, f2 = meshing.extract_udf_mesh(network, n, sparse=True)
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()
    # reported, not asserted: the raw sparse mesh against the truly dense one
    sv, sf = meshing.udf_marching_cubes_sparse(g)
    gdiff = int((g.G[keep].view(torch.int32) != G.reshape(-1, 3)[ids[keep]].view(torch.int32)).any(1).sum())
    if sf.shape == df.shape:
        fdiff = int((sf != df).any(1).sum())
    else:
        fdiff = f"face counts {sf.shape[0]} vs {df.shape[0]}"
    print(f"network N=96 B=8: {g.n_blocks} blocks, {g.n_queried} nodes, {g.n_grad} gradients; holes {holes}; "
          f"brick gradients that differ from the dense grid's: {gdiff}; faces that differ from the dense mesh: {fdiff} "
          f"of {df.shape[0]}")


def test_beyond_the_dense_limit():
    """N = 2049 (the dense entry points stop at 1024): a disc, an open sheet.  Peak memory below one byte per grid node
    (the dense path needs 4 B/node for U alone); the bound is a condition, the expected peak is well under 1 GB."""
    from neuraludf_amd import meshing
    n, rho, c = 2049, 0.3, 0.0123

    def fn(p):
        return S.disc_udf(p, rho, c)
    field = _analytic(fn)
    h = meshing.grid_spacing(*BOX, n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    g = meshing.udf_sparse_grid(field, n, *BOX, block=8, lipschitz=LIP)
    v, f = meshing.udf_marching_cubes_sparse(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"N={n}: {g.n_blocks} of {g.nb ** 3} blocks, {g.n_blocks * 729} brick nodes, {g.n_queried} queried, "
          f"{f.shape[0]} faces, peak {peak / 2 ** 20:.0f} MiB")
    assert peak < n ** 3
    assert 0 < g.n_blocks < g.nb ** 3 // 100
    assert f.shape[0] > 0 and int(f.max()) == v.shape[0] - 1 and int(f.min()) == 0
    v, f = meshing.filter_mesh(v, f, fn(v)[0][:, 0], h)
    vd = v.double()
    a = 0.5 * float(torch.linalg.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]]).norm(dim=1).sum())
    assert 0.95 * math.pi * rho ** 2 <= a <= math.pi * rho ** 2 + 2 * math.pi * rho * h, a
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).sort(1).values
    _, cnt = torch.unique(e[:, 0] * v.shape[0] + e[:, 1], return_counts=True)
    assert int(cnt.max()) <= 2 and bool((cnt == 1).any())


def test_pass_through(network, monkeypatch):
    from neuraludf_amd import meshing
    from neuraludf_amd.train import Trainer
    n = 96
    tr = Trainer(DEV, dict(n_samples=32, n_importance=16, n_outside=8, up_sample_steps=2, perturb=1.0), seed=0)
    v, f = meshing.extract_udf_mesh(tr.udf, n, sparse=True)
    calls = []
    real = meshing.udf_marching_cubes_sparse
    monkeypatch.setattr(meshing, "udf_marching_cubes_sparse", lambda g, **kw: calls.append(g.B) or real(g, **kw))
    vt, ft = tr.extract_udf_mesh(n, sparse=True)
    vr, fr = tr.renderer.extract_udf_geometry(BOX[0], BOX[1], n, sparse=True, block=4)
    v4, f4 = meshing.extract_udf_mesh(tr.udf, n, sparse=True, block=4)
    assert calls == [8, 4, 4]
    assert vt.tobytes() == v.tobytes() and ft.tobytes() == f.tobytes()
    assert vr.tobytes() == v4.tobytes() and fr.tobytes() == f4.tobytes()
    tr.extract_udf_mesh(n)
    assert calls == [8, 4, 4]                                   # dense stays the default


def test_empty_fields_and_argument_errors(network):
    from neuraludf_amd import meshing

    def far(p):                                                # no block is selected
        return torch.full_like(p[:, :1], 5.0), torch.zeros_like(p)

    def flat(p):                                               # every block is selected, no cell is active
        return torch.full_like(p[:, :1], 3.0 * 2 / 31), torch.zeros_like(p)
    for fn, k in ((far, 0), (flat, 64)):
        g = meshing.udf_sparse_grid(_analytic(fn), 32, block=8)
        assert g.n_blocks == k
        v, f = meshing.udf_marching_cubes_sparse(g)
        assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int64 and v.dtype == torch.float32
        with pytest.raises(RuntimeError, match="no surface"):
            meshing.extract_udf_mesh(_analytic(fn), 32, sparse=True)
    with pytest.raises(RuntimeError, match="no surface"):
        meshing.extract_udf_mesh(network, 16, bound_min=(2.0, 2.0, 2.0), bound_max=(3.0, 3.0, 3.0), sparse=True)
    for kw in (dict(block=16), dict(block=0), dict(lipschitz=0.0), dict(lipschitz=float("nan")),
               dict(lipschitz=float("inf"))):
        with pytest.raises(ValueError):
            meshing.extract_udf_mesh(network, 32, sparse=True, **kw)
    for n in (2, 4097):
        with pytest.raises(ValueError):
            meshing.udf_sparse_grid(network, n)
    g = meshing.udf_sparse_grid(_analytic(S.sphere_udf), 32, block=4)
    g.N = 1025
    with pytest.raises(ValueError):
        g.to_dense()
    with pytest.raises(ValueError):
        meshing.udf_marching_cubes_sparse(None)
    U = torch.zeros((1, 1, 1), device=DEV).expand(1025, 1025, 1025)            # the dense limit stays
    with pytest.raises(ValueError):
        meshing.udf_marching_cubes(U, torch.zeros((1, 1, 1, 3), device=DEV).expand(1025, 1025, 1025, 3), *BOX)
