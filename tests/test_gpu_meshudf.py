"""GPU: MeshUDF open-surface meshing (neuraludf_amd/meshing.py, csrc/meshudf.hip) -- the kernels against the numpy
restatement (tests/meshudf_ref.py) bit for bit, analytic fields with known surfaces, the network end to end, and the
argument checks.  What it replaces: the reference's Runner.extract_udf_mesh / extract_mesh.get_mesh_udf_fast."""
import math

import numpy as np
import pytest
import torch

import meshudf_ref as R
from common import build_modules, perturb_

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _points(n, bmin, bmax):
    from neuraludf_amd.models import udf_renderer_blending as rb
    ax = rb._grid_axes(bmin, bmax, n, DEV)
    return ax, torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), -1)


def sphere_field(radius):
    def f(p):
        r = p.norm(dim=-1, keepdim=True)
        return (r - radius).abs()[..., 0], torch.nan_to_num(p / r * torch.sign(r - radius))
    return f


def plane_field(c):
    def f(p):
        dz = p[..., 2:3] - c
        return dz.abs()[..., 0], torch.cat([torch.zeros_like(p[..., :2]), torch.sign(dz)], -1)
    return f


def disc_field(rho, c):
    """distance to the disc x^2 + y^2 <= rho^2, z = c, and its gradient"""
    def f(p):
        s = p[..., :2].norm(dim=-1, keepdim=True)
        dz = p[..., 2:3] - c
        out = (s - rho).clamp_min(0.0)
        u = torch.sqrt(out * out + dz * dz)
        g = torch.cat([out * torch.nan_to_num(p[..., :2] / s), dz], -1) / u
        return u[..., 0], torch.nan_to_num(g)
    return f


def _grid(field, n, bmin, bmax):
    ax, X = _points(n, bmin, bmax)
    U, G = field(X)
    return ax, U.float().contiguous(), G.float().contiguous()


def _mesh(field, n, bmin=BOX[0], bmax=BOX[1]):
    """analytic grid -> udf_marching_cubes -> filter_mesh with the analytic vertex UDF and max_udf = h (numpy out)"""
    from neuraludf_amd import meshing
    _, U, G = _grid(field, n, bmin, bmax)
    v, f = meshing.udf_marching_cubes(U, G, bmin, bmax)
    v, f = meshing.filter_mesh(v, f, field(v)[0], meshing.grid_spacing(bmin, bmax, n))
    return v.cpu().numpy(), f.cpu().numpy()


def _kernel_vs_restatement(ax, U, G, bmin, bmax):
    from neuraludf_amd import meshing
    v, f = meshing.udf_marching_cubes(U, G, bmin, bmax)
    rv, rf = R.marching_cubes(U.cpu().numpy(), G.cpu().numpy(), ax.cpu().numpy(), bmin, bmax)
    assert f.dtype == torch.int64 and v.dtype == torch.float32 and len(rf) > 0
    np.testing.assert_array_equal(f.cpu().numpy(), rf)
    extent = max(b - a for a, b in zip(bmin, bmax))
    assert v.shape == rv.shape
    assert float(np.abs(v.cpu().numpy() - rv).max()) <= 1e-6 * extent
    return len(rf)


def test_kernels_match_restatement_sphere():
    ax, U, G = _grid(sphere_field(0.6), 33, *BOX)
    _kernel_vs_restatement(ax, U, G, *BOX)


def test_kernels_match_restatement_disc_non_cubic_box():
    bmin, bmax = (-0.8, -0.7, -0.5), (0.9, 0.75, 0.6)
    ax, U, G = _grid(disc_field(0.45, 0.0371), 40, bmin, bmax)
    _kernel_vs_restatement(ax, U, G, bmin, bmax)


def test_kernels_match_restatement_random_fields():
    """random U in [0, 1.2 h] and random G: nearly every cell active, every kind of case, ambiguous faces included"""
    from neuraludf_amd import meshing
    n = 24
    h = meshing.grid_spacing(*BOX, n)
    g = torch.Generator().manual_seed(5)
    U = (torch.rand((n, n, n), generator=g) * (1.2 * h)).to(DEV)
    G = torch.randn((n, n, n, 3), generator=g).to(DEV)
    ax, _ = _points(n, *BOX)
    assert _kernel_vs_restatement(ax, U, G, *BOX) > 1000


def test_kernels_match_restatement_network_grid():
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    udf = perturb_(build_modules(fields, seed=0))["udf"].to(DEV)
    U, G = meshing.udf_grid(udf, 48)
    ax, _ = _points(48, *BOX)
    _kernel_vs_restatement(ax, U, G, *BOX)


def test_plane_is_one_sheet():
    n, c = 65, 0.013                         # nodes at multiples of 1/32: c is off them
    v, f = _mesh(plane_field(c), n)
    assert len(f) == 2 * (n - 1) ** 2
    assert float(np.abs(v[:, 2] - c).max()) <= 1e-6
    _, cnt = R.edge_counts(f)
    assert int((cnt == 1).sum()) == 4 * (n - 1) and cnt.max() == 2


def test_sphere_is_closed():
    from neuraludf_amd import meshing
    n, radius = 128, 0.6
    v, f = _mesh(sphere_field(radius), n)
    _, cnt = R.edge_counts(f)
    assert (cnt == 2).all()
    assert R.euler(len(v), f) == 2
    assert R.components(len(v), f) == 1
    assert abs(R.area(v, f) / (4 * math.pi * radius ** 2) - 1) < 0.02
    h = meshing.grid_spacing(*BOX, n)
    assert float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - radius).max()) < 0.05 * h


def test_disc_is_an_open_sheet():
    from neuraludf_amd import meshing
    n, rho, c = 96, 0.5, 0.0123
    h = meshing.grid_spacing(*BOX, n)
    v, f = _mesh(disc_field(rho, c), n)
    a = R.area(v, f)
    # a threshold iso-surface of the UDF would be a closed double layer: about 2 pi rho^2
    assert 0.95 * math.pi * rho ** 2 <= a <= math.pi * rho ** 2 + 2 * math.pi * rho * h
    cen = v.astype(np.float64)[f].mean(1)
    assert float(np.linalg.norm(cen[:, :2], axis=1).max()) <= rho + h
    _, cnt = R.edge_counts(f)
    assert cnt.max() <= 2 and (cnt == 1).any()


def test_network_end_to_end():
    """the unperturbed geometric init of the shipped DTU conf (bias 0.5, udf_type abs).  Two expectations of the issue are
    replaced by what the CPU oracle (oracle.udf_oracle.udf_forward / udf_gradient, same seed-0 weights) shows:
      * radius: the init's zero level is not the radius-0.5 sphere.  The minimum of the oracle's UDF along 3000 random rays
        from the origin lies at radii 0.235 .. 0.391 (radial step 0.001; minimum UDF <= 6e-4 on every ray).  The band
        asserted is that one widened by 2 h (h = 2/95) for the vertices' distance from the zero level.
      * chi = 2: the init is steeper than a distance (|grad U| up to 1.22 in the band U < 2 h), so a few cells the surface
        crosses have a corner value above the active test's 1.74 h and emit nothing.  On the oracle's grid the numpy
        restatement leaves 14 holes of one triangle each (42 boundary edges, chi = -12) -- the holes the reference's
        trimesh fill_holes() closes, which stays out of scope.  Asserted: one component, genus 0 (chi = 2 - holes), and
        every hole a single missing triangle."""
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    from neuraludf_amd.models.udf_renderer_blending import extract_fields
    from neuraludf_amd.train import Trainer
    n = 96
    udf = build_modules(fields, seed=0)["udf"].to(DEV)
    v, f = meshing.extract_udf_mesh(udf, n)
    assert v.dtype == np.float32 and f.dtype == np.int64
    _, cnt = R.edge_counts(f)
    n_boundary, holes = R.boundary_loops(len(v), f)
    assert cnt.max() == 2 and R.components(len(v), f) == 1
    assert R.euler(len(v), f) == 2 - holes and n_boundary == 3 * holes and holes <= 20, (n_boundary, holes)
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert 0.235 - 0.043 <= r.min() and r.max() <= 0.391 + 0.043, (r.min(), r.max())
    U, _ = meshing.udf_grid(udf, n)
    np.testing.assert_array_equal(U.cpu().numpy(), extract_fields(BOX[0], BOX[1], n, lambda p: udf.udf(p)[:, 0], DEV))
    v2, f2 = meshing.extract_udf_mesh(udf, n)
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()

    tr = Trainer(DEV, dict(n_samples=32, n_importance=16, n_outside=8, up_sample_steps=2, perturb=1.0), seed=0)
    S = np.diag([2.5, 2.5, 2.5, 1.0])
    S[:3, 3] = [0.3, -1.2, 4.0]
    vn, fn = tr.extract_udf_mesh(n)
    vw, fw = tr.extract_udf_mesh(n, world_space=True, scale_mat=S)
    np.testing.assert_array_equal(fw, fn)
    np.testing.assert_array_equal(vw, (vn * S[0, 0] + S[:3, 3][None]).astype(np.float32))
    vr, fr = tr.renderer.extract_udf_geometry(BOX[0], BOX[1], n)
    np.testing.assert_array_equal(vr, vn)
    np.testing.assert_array_equal(fr, fn)


def test_large_grid_64bit_paths():
    """N = 512, the largest grid of the suite (4.0e8 edge flags and their int64 scan): the sphere stays closed"""
    from neuraludf_amd import meshing
    n = 512
    _, U, G = _grid(sphere_field(0.6), n, *BOX)
    v, f = meshing.udf_marching_cubes(U, G, *BOX)
    del U, G
    f = f.cpu().numpy()
    assert int(f.max()) == len(v) - 1
    assert R.euler(len(v), f) == 2
    _, cnt = R.edge_counts(f)
    assert (cnt == 2).all()


def test_argument_errors_and_empty_fields():
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    for n in (2, 1025):
        U = torch.zeros((1, 1, 1), device=DEV).expand(n, n, n)
        G = torch.zeros((1, 1, 1, 3), device=DEV).expand(n, n, n, 3)
        with pytest.raises(ValueError):
            meshing.udf_marching_cubes(U, G, *BOX)
    U, G = torch.zeros((8, 8, 8), device=DEV), torch.zeros((8, 8, 8, 3), device=DEV)
    for bad in [(U.double(), G), (U, G.half()), (U.cpu(), G.cpu()), (U, G.cpu()), (U, G[:7]), (U[:, :, :7], G),
                (U[..., None], G)]:
        with pytest.raises(ValueError):
            meshing.udf_marching_cubes(*bad, *BOX)
    udf = build_modules(fields, seed=0)["udf"].to(DEV)
    with pytest.raises(ValueError):
        meshing.udf_grid(udf, 2)
    # a field with no surface: empty arrays from the mesher, RuntimeError from the one-call API
    v, f = meshing.udf_marching_cubes(U + 1.0, G, *BOX)
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int64
    with pytest.raises(RuntimeError, match="no surface"):
        meshing.extract_udf_mesh(udf, 16, bound_min=(2.0, 2.0, 2.0), bound_max=(3.0, 3.0, 3.0))
