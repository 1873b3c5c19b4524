"""GPU: the face orientation and the vertex normals (neuraludf_amd/meshclean.py orient_faces / vertex_normals,
csrc/meshorient.hip) against the numpy restatement (tests/meshorient_ref.py): faces, flipped, labels and orientable bit
for bit, the normals to the float64 / float32 bounds worked out below -- plus the mesher end to end, the PLY files, the
CLI and the argument checks.  What it adds to the reference: extract_mesh.py:218-219 leaves the winding alone, and
extract_mesh.py:272-275 takes the normals from trimesh."""
import numpy as np
import pytest
import torch

import meshorient_ref as O
import meshudf_ref as R
from common import build_modules

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
# float64 normals: the terms differ from the restatement's by a few ulps of atan2 (<= 1e-15 each, theta <= pi), a vertex
# has fewer than 16 corners, and the sum is divided by its length |N_v| -- asserted to be > 0.05 where this bound is used:
# 16 * 1e-15 / 0.05 = 3.2e-13 < 1e-12.  float32: two ulps at 1 (2^-23 each): one for a rounding boundary, one of margin.
TOL64, TOL32, MIN_LENGTH = 1e-12, 2.4e-7, 0.05


def _points(n):
    from neuraludf_amd.models import udf_renderer_blending as rb
    ax = rb._grid_axes(BOX[0], BOX[1], n, DEV)
    return torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), -1)


def sphere_field(radius):
    def f(p):
        r = p.norm(dim=-1, keepdim=True)
        return (r - radius).abs()[..., 0], torch.nan_to_num(p / r * torch.sign(r - radius))
    return f


def disc_field(rho, c):
    def f(p):
        s = p[..., :2].norm(dim=-1, keepdim=True)
        dz = p[..., 2:3] - c
        out = (s - rho).clamp_min(0.0)
        u = torch.sqrt(out * out + dz * dz)
        g = torch.cat([out * torch.nan_to_num(p[..., :2] / s), dz], -1) / u
        return u[..., 0], torch.nan_to_num(g)
    return f


def _mesh(field, n):
    """analytic grid -> udf_marching_cubes -> filter_mesh (device tensors)"""
    from neuraludf_amd import meshing
    U, G = field(_points(n))
    v, f = meshing.udf_marching_cubes(U.float().contiguous(), G.float().contiguous(), *BOX)
    return meshing.filter_mesh(v, f, field(v)[0], meshing.grid_spacing(*BOX, n))


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                   # a copy: the fixtures' arrays are read-only


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def sphere():
    """the GPU mesher's N = 33 sphere and the restatement's answers for it, computed once"""
    vt, ft = _mesh(sphere_field(0.6), 33)
    v, f = _frozen(vt.cpu().numpy(), ft.cpu().numpy())
    assert R.is_closed_manifold(f) and R.euler(len(v), f) == 2
    return dict(v=v, f=f, default=_frozen(*O.orient(v, f)), outward=_frozen(*O.orient(v, f, (0.0, 0.0, 0.0))))


@pytest.fixture(scope="module")
def mixed(sphere):
    vt, ft = _mesh(disc_field(0.5, 0.0123), 48)
    v, f = _frozen(*O.mixed_mesh((sphere["v"], sphere["f"]), (vt.cpu().numpy(), ft.cpu().numpy())))
    origin = (0.05, -0.02, 0.3)
    return dict(v=v, f=f, origin=origin, default=_frozen(*O.orient(v, f)), outward=_frozen(*O.orient(v, f, origin)))


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("faces", "flipped", "labels", "orientable")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("mode", ["default", "outward"])
def test_sphere_is_oriented(sphere, mode):
    from neuraludf_amd import meshing
    v, f = sphere["v"], sphere["f"]
    origin = (0.0, 0.0, 0.0) if mode == "outward" else None
    info = {}
    got = meshing.orient_faces(_dev(v), _dev(f), origin, _info=info)
    assert isinstance(got, meshing.Orientation)
    assert got.faces.dtype == got.labels.dtype == torch.int64 and got.flipped.dtype == got.orientable.dtype == torch.bool
    _assert_equal(got, sphere[mode])
    out = got.faces.cpu().numpy()
    n_flipped = int(got.flipped.sum())
    print(f"sphere {mode}: {n_flipped} of {len(f)} faces flipped, {info['rounds']} rounds, "
          f"{O.incompatible_edges(f)} of {len(O.manifold_edges(f))} edges incompatible before")
    assert n_flipped > 0 and O.incompatible_edges(f) > 0 and O.incompatible_edges(out) == 0
    assert info["components"] == info["orientable"] == 1 and info["non_orientable"] == 0 and info["flipped"] == n_flipped
    assert bool(got.orientable.all()) and bool((got.labels == 0).all())
    if mode == "default":
        assert 2 * n_flipped <= len(f)
    else:
        assert O.signed_volume(v, out) > 0
    again = meshing.orient_faces(_dev(v), _dev(f), origin)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # float32 vertices and a tensor as the point
    if origin is not None:
        got32 = meshing.orient_faces(_dev(v.astype(np.float32)), _dev(f), torch.zeros(3))
        assert torch.equal(got32.faces, got.faces)


@pytest.mark.parametrize("mode", ["default", "outward"])
def test_mixed_mesh(mixed, mode):
    from neuraludf_amd import meshing
    v, f = mixed["v"], mixed["f"]
    info = {}
    got = meshing.orient_faces(_dev(v), _dev(f), mixed["origin"] if mode == "outward" else None, _info=info)
    want = mixed[mode]
    _assert_equal(got, want)
    labels, orientable = want[2], want[3]
    print(f"mixed {mode}: {len(f)} faces, {info}")
    assert info["components"] == len(set(labels.tolist())) and info["non_orientable"] == 1
    assert info["orientable"] == info["components"] - 1 and info["flipped"] == int(want[1].sum()) > 0
    assert int((~orientable).sum()) == 24                                  # the band, returned as it came
    np.testing.assert_array_equal(got.faces.cpu().numpy()[~orientable], f[~orientable])
    assert O.incompatible_edges(got.faces.cpu().numpy(), orientable) == 0
    # the three faces on one edge are three components, the face with a repeated vertex one more and never flipped
    repeated = np.nonzero((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))[0]
    assert len(repeated) == 1 and labels[repeated[0]] == repeated[0] and not want[1][repeated[0]]
    assert int((np.bincount(labels, minlength=len(f)) == 1).sum()) >= 4


def test_strip_of_20000_faces_numbered_at_random():
    from neuraludf_amd import meshing
    v, f = O.strip(20000, seed=0)
    want = O.orient(v, f)
    info = {}
    got = meshing.orient_faces(_dev(v), _dev(f), _info=info)
    print(f"strip of {len(f)} faces numbered at random: {info['rounds']} rounds, {info['flipped']} flipped")
    _assert_equal(got, want)
    assert 1 <= info["rounds"] <= len(f) and info["components"] == 1 and info["non_orientable"] == 0
    assert O.incompatible_edges(got.faces.cpu().numpy()) == 0
    # numbered along the strip and wound consistently: nothing to do
    v, f = O.strip(20000)
    got = meshing.orient_faces(_dev(v), _dev(f), _info=info)
    print(f"strip in order: {info['rounds']} rounds")
    assert not bool(got.flipped.any()) and torch.equal(got.faces, _dev(f)) and bool((got.labels == 0).all())


def _check_normals(v, f, min_cos_radial=None):
    from neuraludf_amd import meshing
    want, length = O.vertex_normals(v, f, return_length=True)
    used = np.zeros(len(v), dtype=bool)
    used[f.reshape(-1)] = True
    assert length[used].min() > MIN_LENGTH and (length[~used] == 0).all()
    got64 = meshing.vertex_normals(_dev(v), _dev(f), torch.float64)
    got32 = meshing.vertex_normals(_dev(v), _dev(f))
    assert got64.dtype == torch.float64 and got32.dtype == torch.float32 and got64.shape == got32.shape == (len(v), 3)
    got64, got32 = got64.cpu().numpy(), got32.cpu().numpy()
    e64, e32 = np.abs(got64 - want).max(), np.abs(got32.astype(np.float64) - want).max()
    print(f"normals of {len(v)} vertices: max |float64 - restatement| {e64:.3e}, float32 {e32:.3e}")
    assert e64 <= TOL64 and e32 <= TOL32
    assert (got64[~used] == 0).all() and (got32[~used] == 0).all()
    np.testing.assert_allclose(np.linalg.norm(got64[used], axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got32, got64.astype(np.float32))             # computed in float64, cast at the end
    if min_cos_radial is not None:
        cos = np.einsum("ij,ij->i", got64, v / np.linalg.norm(v, axis=1, keepdims=True))
        print(f"min cosine against the radial direction {cos.min():.5f}")
        assert cos.min() >= min_cos_radial


def test_vertex_normals(sphere, mixed):
    _check_normals(sphere["v"].astype(np.float64), sphere["outward"][0], min_cos_radial=0.99)
    _check_normals(mixed["v"], mixed["outward"][0])


def test_vertex_normals_of_slivers_stay_finite():
    from neuraludf_amd import meshing
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 1e-300, 0], [0.5, 1e-9, 1e-12], [0, 1, 0], [1e200, 0, 0],
                  [0, 1e200, 0], [3, 3, 3], [1, 1e-160, 0]], dtype=np.float64)
    f = np.array([[0, 1, 2],              # three points on a line: zero area
                  [0, 1, 3],              # a sliver: |n|^2 underflows to 0
                  [0, 1, 4],              # a near-sliver
                  [0, 1, 5],
                  [0, 6, 7],              # the cross product overflows: not finite, contributes nothing
                  [1, 1, 5],              # a repeated vertex
                  [0, 1, 9]])             # |n|^2 is subnormal
    for dtype in (torch.float64, torch.float32):
        n = meshing.vertex_normals(_dev(v), _dev(f), dtype).cpu().numpy().astype(np.float64)
        assert np.isfinite(n).all()
        length = np.linalg.norm(n, axis=1)
        assert (np.isclose(length, 1.0, rtol=0, atol=1e-6) | (length == 0)).all()
        assert (n[8] == 0).all() and length[5] > 0
    np.testing.assert_allclose(meshing.vertex_normals(_dev(v), _dev(f), torch.float64).cpu().numpy(), O.vertex_normals(v, f),
                               rtol=0, atol=1e-9)


def test_extract_udf_mesh_orients_as_its_last_step():
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    udf = build_modules(fields, seed=0)["udf"].to(DEV)
    v0, f0 = meshing.extract_udf_mesh(udf, 33, fill_holes=True)
    v1, f1 = meshing.extract_udf_mesh(udf, 33, fill_holes=True, orient=False)
    assert v1.tobytes() == v0.tobytes() and f1.tobytes() == f0.tobytes()
    origin = (0.0, 0.0, 0.0)
    v, f = meshing.extract_udf_mesh(udf, 33, fill_holes=True, orient=True, outward_from=origin)
    assert v.shape == v0.shape and f.shape == f0.shape and v.tobytes() == v0.tobytes()
    want, flipped, labels, orientable = O.orient(v0, f0, origin)
    print(f"network at N = 33: {len(f0)} faces, {int(flipped.sum())} flipped, {len(set(labels.tolist()))} components, "
          f"{O.incompatible_edges(f0)} incompatible edges before")
    np.testing.assert_array_equal(f, want)
    assert orientable.any() and O.incompatible_edges(f0) > 0 and O.incompatible_edges(f, orientable) == 0
    np.testing.assert_array_equal(np.sort(f, 1), np.sort(f0, 1))
    v2, f2 = meshing.extract_udf_mesh(udf, 33, fill_holes=True, orient=True)
    np.testing.assert_array_equal(f2, O.orient(v0, f0)[0])
    _, f3 = meshing.extract_udf_mesh(udf, 33, fill_holes=True, outward_from=origin)          # implies orient
    assert f3.tobytes() == f.tobytes()


def test_ply_files_and_cli(tmp_path, sphere, capsys):
    from neuraludf_amd import meshing
    v, f = sphere["v"], sphere["f"]
    n = meshing.vertex_normals(_dev(v), _dev(sphere["outward"][0])).cpu().numpy()
    meshing.write_ply(tmp_path / "plain.ply", v, f)
    meshing.write_ply(tmp_path / "normals.ply", v, f, n)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode()
    rec = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"], rec["v"] = 3, f
    assert (tmp_path / "plain.ply").read_bytes() == head + v.astype("<f4").tobytes() + rec.tobytes()
    assert len(meshing.read_ply(tmp_path / "plain.ply")) == len(meshing.read_ply(tmp_path / "normals.ply")) == 2
    rv, rf, rn = meshing.read_ply(tmp_path / "normals.ply", with_normals=True)
    np.testing.assert_array_equal(rv, v.astype(np.float64))
    np.testing.assert_array_equal(rf, f)
    assert rn.dtype == np.float64 and rn.astype(np.float32).tobytes() == n.tobytes()
    rv, rf, rn = meshing.read_ply(tmp_path / "plain.ply", with_normals=True)
    assert rn is None and rv.shape == v.shape
    with pytest.raises(ValueError):
        meshing.write_ply(tmp_path / "bad.ply", v, f, n[:-1])
    # the CLI: orientation, then normals computed after all other steps
    assert meshing.main([str(tmp_path / "plain.ply"), str(tmp_path / "out.ply"), "--orient", "--normals"]) == 0
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("orient:")]
    want_f, want_flipped, _, _ = sphere["default"]
    assert line == [f"orient: 1 components, 0 not orientable, {int(want_flipped.sum())} faces flipped"]
    ov, of, on = meshing.read_ply(tmp_path / "out.ply", with_normals=True)
    np.testing.assert_array_equal(of, want_f)
    np.testing.assert_array_equal(ov, v.astype(np.float64))
    assert np.abs(on - O.vertex_normals(v, want_f)).max() <= TOL32
    assert meshing.main([str(tmp_path / "plain.ply"), str(tmp_path / "out2.ply"), "--outward-from", "0", "0", "0"]) == 0
    assert "orient:" in capsys.readouterr().out
    ov, of, on = meshing.read_ply(tmp_path / "out2.ply", with_normals=True)
    np.testing.assert_array_equal(of, sphere["outward"][0])
    assert on is None
    assert meshing.main([str(tmp_path / "plain.ply"), str(tmp_path / "out3.ply")]) == 0            # no flag: as before
    assert "orient:" not in capsys.readouterr().out
    assert (tmp_path / "out3.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()


def test_argument_errors_and_empty_meshes():
    from neuraludf_amd import meshing
    v = torch.zeros((4, 3), device=DEV)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], device=DEV)
    for bad_v, bad_f in [(v, f.int()), (v, f.cpu()), (v.cpu(), f), (v, f[:, :2]), (v[:, :2], f), (v.half(), f), (v[:3], f),
                         (v, f - 1), (v.cpu().numpy(), f), (v, f.cpu().numpy())]:
        with pytest.raises(ValueError):
            meshing.orient_faces(bad_v, bad_f)
        with pytest.raises(ValueError):
            meshing.vertex_normals(bad_v, bad_f)
    for origin in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0), "abc", 1.0,
                   ("a", "b", "c")):
        with pytest.raises(ValueError):
            meshing.orient_faces(v, f, origin)
    for dtype in (torch.float16, torch.int64, None):
        with pytest.raises(ValueError):
            meshing.vertex_normals(v, f, dtype)
    e = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    for vv in (v, v[:0]):
        info = {}
        got = meshing.orient_faces(vv, e, (0.0, 0.0, 0.0), _info=info)
        assert got.faces.shape == (0, 3) and got.faces.dtype == torch.int64 and info["rounds"] == info["components"] == 0
        assert got.flipped.shape == got.labels.shape == got.orientable.shape == (0,)
        assert got.flipped.dtype == got.orientable.dtype == torch.bool and got.labels.dtype == torch.int64
        n = meshing.vertex_normals(vv, e)
        assert n.shape == vv.shape and n.dtype == torch.float32 and not bool(n.any())
    # faces that share no manifold edge: no round, every face its own component
    got = meshing.orient_faces(v, f[:1], _info=info)
    assert info["rounds"] == 0 and got.labels.tolist() == [0] and not bool(got.flipped.any())
