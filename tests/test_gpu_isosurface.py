"""GPU: level-set meshing (neuraludf_amd/meshing.py iso_marching_cubes / iso_sparse_grid / iso_marching_cubes_sparse /
extract_iso_mesh, csrc/isosurface.hip) -- the kernels against the numpy restatement (tests/isosurface_ref.py), the sparse
mesher against the dense one on the same values, order included, the properties of the meshes, 64-bit ids beyond the
dense limit, and the reference's call surface (extract_geometry without PyMCubes, Trainer.validate_mesh)."""
import math
import sys

import numpy as np
import pytest
import torch

import isosurface_ref as I
import meshudf_ref as R
from common import build_modules, perturb_

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = I.BOX
CASES = ("sphere33", "slab40_noncubic", "random24", "network48", "sphere50_ragged")


@pytest.fixture(scope="module")
def cases():
    """name -> (query_func, dense F [N, N, N] on the GPU, N, box, level, a lipschitz bound that holds for the field); every
    grid is computed once and left unchanged"""
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    from neuraludf_amd.models import udf_renderer_blending as rb
    out = {}
    for name, fn, n, box, level in (("sphere33", I.sphere_sdf, 33, BOX, 0.0), ("slab40_noncubic", I.slab_sdf, 40, I.NONCUBIC, 0.03),
                                    ("sphere50_ragged", I.sphere_sdf, 50, BOX, 0.0)):
        out[name] = (fn, rb._grid_query_device(*box, n, fn, DEV, 1), n, box, level, 1.05)
    F = I.random_field_with_specials(24, 11, 0.5).to(DEV)
    out["random24"] = (I.TableQuery(F, *BOX), F, 24, BOX, 0.5, 100.0)         # lipschitz 100: every block is selected
    udf = perturb_(build_modules(fields, seed=0))["udf"].to(DEV)
    F = meshing.udf_values(udf, 48, *BOX)
    out["network48"] = (I.TableQuery(F, *BOX), F, 48, BOX, 0.02, 2.0)
    return out


@pytest.fixture(scope="module")
def dense_meshes(cases):
    from neuraludf_amd import meshing
    return {k: meshing.iso_marching_cubes(F, level, *box) for k, (_, F, _, box, level, _) in cases.items()}


@pytest.mark.parametrize("name", CASES[:4])
def test_kernels_match_restatement(cases, dense_meshes, name):
    from neuraludf_amd.models import udf_renderer_blending as rb
    _, F, n, box, level, _ = cases[name]
    v, f = dense_meshes[name]
    rv, rf = I.marching_cubes(F.cpu().numpy(), level, rb._grid_axes(*box, n, DEV).cpu().numpy())
    assert f.dtype == torch.int64 and v.dtype == torch.float32 and len(rf) > (1000 if name == "random24" else 0)
    np.testing.assert_array_equal(f.cpu().numpy(), rf)
    extent = max(b - a for a, b in zip(*box))
    assert v.shape == rv.shape
    err = float(np.abs(v.cpu().numpy() - rv).max())
    print(f"{name}: {len(rf)} faces, {len(rv)} vertices, largest vertex difference {err:.3g}")
    assert err <= 1e-6 * extent


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("name", CASES)
def test_sparse_equals_dense_on_the_same_values(cases, dense_meshes, name, b):
    from neuraludf_amd import meshing
    query, F, n, box, level, lip = cases[name]
    g = meshing.iso_sparse_grid(query, n, level, *box, block=b, lipschitz=lip, device=DEV)
    blocks = I.select(g.coarse.cpu().numpy(), n, b, *I.selection_bounds(*box, n, level, b, lip))
    np.testing.assert_array_equal(g.blocks.cpu().numpy(), blocks)
    if name == "random24":
        assert g.n_blocks == g.nb ** 3
    ids = g.node_ids()
    keep = ids >= 0
    assert torch.equal(g.F[keep].view(torch.int32), F.reshape(-1)[ids[keep]].view(torch.int32))
    assert bool(torch.isinf(g.F[~keep]).all())
    v, f = meshing.iso_marching_cubes_sparse(g, level)
    dv, df = dense_meshes[name]
    print(f"{name} B={b}: {g.n_blocks} of {g.nb ** 3} blocks, {f.shape[0]} faces, {v.shape[0]} vertices")
    assert f.shape[0] > 0 and f.dtype == torch.int64 and v.dtype == torch.float32
    assert torch.equal(f, df)
    assert torch.equal(v.view(torch.int32), dv.view(torch.int32))
    assert int(f.min()) >= 0 and int(f.max()) == v.shape[0] - 1 and bool(torch.isfinite(v).all())


def test_sphere_properties():
    from neuraludf_amd import meshing
    n, radius = 64, 0.6
    v, f = meshing.extract_iso_mesh(I.sphere_sdf, n, 0.0, device=DEV)
    assert v.dtype == np.float32 and f.dtype == np.int64
    h = 2.0 / (n - 1)
    assert R.is_closed_manifold(f) and I.directed_edges_unique(f)
    assert R.euler(len(v), f) == 2 and R.components(len(v), f) == 1
    area, vol = R.area(v, f), I.signed_volume(v, f)
    err = float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - radius).max())
    print(f"area ratio {area / (4 * math.pi * radius ** 2):.4f}, volume ratio {vol / (4 / 3 * math.pi * radius ** 3):.4f}, "
          f"radial error {err / h:.4f} h")
    assert abs(area / (4 * math.pi * radius ** 2) - 1) <= 0.01
    assert vol > 0 and abs(vol / (4 / 3 * math.pi * radius ** 3) - 1) <= 0.01
    assert err <= 0.05 * h
    # the shell {udf = 0.05} of the unsigned field, with the component filter
    sv, sf = meshing.extract_iso_mesh(I.shell_udf, n, 0.05, device=DEV)
    assert R.is_closed_manifold(sf) and R.components(len(sv), sf) == 2 and R.euler(len(sv), sf) == 4
    kv, kf = meshing.extract_iso_mesh(I.shell_udf, n, 0.05, keep_largest=True, device=DEV)
    assert R.components(len(kv), kf) == 1 and R.euler(len(kv), kf) == 2 and 0 < len(kf) < len(sf)
    assert abs(np.linalg.norm(kv.astype(np.float64), axis=1).mean() - (radius + 0.05)) < h


def test_random_field_is_closed_and_consistently_wound():
    from neuraludf_amd import meshing
    F = I.random_field(24, 3, raise_boundary=True).to(DEV)
    v, f = meshing.iso_marching_cubes(F, 0.5, *BOX)
    f = f.cpu().numpy()
    assert len(f) > 1000 and f.max() == v.shape[0] - 1
    _, cnt = R.edge_counts(f)
    assert (cnt == 2).all() and I.directed_edges_unique(f)


def _edge_counts(f, n_verts):
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).sort(1).values
    return torch.unique(e[:, 0] * n_verts + e[:, 1], return_counts=True)[1]


def test_ids_beyond_32_bits():
    """N = 1025 (above the dense limit; edge ids 3 N^3 > 2^31): a closed sphere from O(surface) blocks.  A selected
    block has a coarse corner within lipschitz r of the sphere; that shell holds 4 pi R^2 * 2 lipschitz r / (8 h)^3 =
    8.4 k coarse nodes with 8 blocks each, 67 k blocks of the 2.1 M, which bounds the brick and coarse storage."""
    from neuraludf_amd import meshing
    n, b, radius = 1025, 8, 0.3
    g = meshing.iso_sparse_grid(lambda p: I.sphere_sdf(p, radius), n, 0.0, *BOX, block=b, lipschitz=1.05, device=DEV)
    v, f = meshing.iso_marching_cubes_sparse(g, 0.0)
    print(f"N={n}: {g.n_blocks} of {g.nb ** 3} blocks, {g.n_queried} nodes queried, {f.shape[0]} faces")
    assert (g.nb, g.coarse.numel(), g.block_slot.numel()) == (128, 129 ** 3, 128 ** 3)
    assert 0 < g.n_blocks <= 67000 and g.F.shape == (g.n_blocks, 729) and g.n_queried <= g.n_blocks * 729
    assert f.shape[0] > 0 and int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1 and bool(torch.isfinite(v).all())
    cnt = _edge_counts(f, v.shape[0])
    assert bool((cnt == 2).all())
    assert v.shape[0] - cnt.numel() + f.shape[0] == 2
    assert float((v.double().norm(dim=1) - radius).abs().max()) <= 0.05 * 2.0 / (n - 1)


@pytest.fixture(scope="module")
def trainer():
    from neuraludf_amd.train import Trainer
    return Trainer(DEV, dict(n_samples=32, n_importance=16, n_outside=8, up_sample_steps=2, perturb=1.0), seed=0)


def test_extract_geometry_without_pymcubes(trainer, monkeypatch):
    monkeypatch.setitem(sys.modules, "mcubes", None)
    n, thr = 96, 0.02
    h = 2.0 / (n - 1)
    v, t = trainer.renderer.extract_geometry(BOX[0], BOX[1], n, threshold=thr)
    assert v.dtype == np.float64 and v.shape[1] == 3 and t.dtype == np.int64 and t.shape[1] == 3 and len(t) > 0
    assert t.min() == 0 and t.max() == len(v) - 1
    _, cnt = R.edge_counts(t)
    assert cnt.max() <= 2
    with torch.no_grad():
        u = trainer.udf.udf(torch.from_numpy(v).float().to(DEV))[:, 0]
    off = float((u - thr).abs().max())
    print(f"N={n}: {len(t)} faces, |udf - threshold| at the vertices <= {off / h:.3f} h")
    assert off <= 2.0 * h
    v2, t2 = trainer.renderer.extract_geometry(BOX[0], BOX[1], n, threshold=thr)
    assert v.tobytes() == v2.tobytes() and t.tobytes() == t2.tobytes()
    for kw in (dict(mesher="gpu"), dict(mesher="gpu", sparse=True), dict(mesher="gpu", sparse=True, block=4)):
        vs, ts = trainer.renderer.extract_geometry(BOX[0], BOX[1], n, threshold=thr, **kw)
        assert v.tobytes() == vs.tobytes() and t.tobytes() == ts.tobytes(), kw
    S = np.diag([2.5, 2.5, 2.5, 1.0])
    S[:3, 3] = [0.1, -0.2, 0.3]
    vw, tw = trainer.validate_mesh(n, thr, world_space=True, scale_mat=S)
    assert vw.dtype == np.float64 and vw.tobytes() == (v * S[0, 0] + S[:3, 3][None]).tobytes() and tw.tobytes() == t.tobytes()
    vb, tb = trainer.validate_mesh(n, thr, sparse=True)
    assert vb.tobytes() == v.tobytes() and tb.tobytes() == t.tobytes()
    with pytest.raises(ValueError):
        trainer.validate_mesh(n, thr, world_space=True)
    with pytest.raises(ImportError):
        trainer.renderer.extract_geometry(BOX[0], BOX[1], n, threshold=thr, mesher="mcubes")
    with pytest.raises(ValueError, match="mesher"):
        trainer.renderer.extract_geometry(BOX[0], BOX[1], n, threshold=thr, mesher="cpu")
    for kw in (dict(), dict(sparse=True)):
        with pytest.raises(RuntimeError, match="no surface"):
            trainer.renderer.extract_geometry(BOX[0], BOX[1], 32, threshold=50.0, mesher="gpu", **kw)


def test_empty_inputs():
    from neuraludf_amd import meshing
    v, f = meshing.iso_marching_cubes(torch.zeros((0, 0, 0), device=DEV), 0.0, *BOX)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64
    v, f = meshing.iso_marching_cubes(torch.ones((5, 5, 5), device=DEV), 0.0, *BOX)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    g = meshing.iso_sparse_grid(lambda p: torch.full_like(p[:, 0], 5.0), 32, 0.0, *BOX, device=DEV)
    assert g.n_blocks == 0
    v, f = meshing.iso_marching_cubes_sparse(g, 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64
    with pytest.raises(ValueError):
        meshing.iso_marching_cubes(torch.zeros((1, 1, 1), device=DEV).expand(1025, 1025, 1025), 0.0, *BOX)
