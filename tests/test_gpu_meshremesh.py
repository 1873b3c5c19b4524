"""GPU: isotropic remeshing (neuraludf_amd/meshclean.py remesh_isotropic, csrc/meshremesh.hip) against the numpy restatement
(tests/meshremesh_ref.py), bit for bit: each entry point through the descriptor, then the driver with and without the
projection -- plus two runs, the independence of the winding and of the order of the faces, the output vertices against the
exact point-to-mesh distance, the mesher end to end and the CLI.

The distance cap.  A projected vertex is closest_on_mesh's `point`, a float64 combination of one face's corners: asked for
its distance to the same mesh, closest_on_mesh finds that face or a neighbour a few u of the coordinates' size away (u =
2^-52).  The issue holds it to 1e-12 of the bounding box's diagonal, the cap of tests/test_gpu_meshsubdiv.py; the test
prints what it measures."""
import math

import numpy as np
import pytest
import torch

import meshremesh_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
NAMES = ("ico0", "fan", "three", "awkward", "sheet", "stretched", "cube", "sphere", "squashed_ico2")
EXTRA = dict(jittered=R.jittered_sheet, dented=R.dented_disk, tetrahedron=R.tetrahedron)     # statuses the nine do not reach
FACTORS = (0.5, 1.0, 1.5)
COS30 = math.cos(math.radians(30.0))


@pytest.fixture(scope="module", autouse=True)
def _hand_back_the_cache():
    """these tests leave float64 geometry in the blocks torch's allocator keeps; hand the blocks back, as
    tests/test_gpu_meshsmooth.py does"""
    yield
    torch.cuda.empty_cache()


def _frozen(v, f):
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


MESHES = {k: _frozen(*m) for k, m in R.meshes().items()}
MESHES.update({k: _frozen(*make()) for k, make in EXTRA.items()})
MEAN = {k: R.mean_edge(v, f) for k, (v, f) in MESHES.items()}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # a copy: the fixtures' arrays are read-only


def _host(t):
    return t.cpu().numpy()


class _Kernels:
    """the six entry points on a mesh, through the descriptor, as the driver calls them; outputs preset to a sentinel"""

    def __init__(self, v, f):
        from neuraludf_amd import _lib, meshclean
        self.lib, self.pos, self.faces = _lib, _dev(v), _dev(f)
        self.t = meshclean._remesh_tables(self.pos, self.faces)
        self.d, self.n_verts, self.n_edges = self.t.d, len(v), self.t.table.edges.shape[0]

    def _out(self, shape, dtype, fill=-7):
        return torch.full(shape, fill, dtype=dtype, device=DEV)

    def collapse_check(self, low, high, cos_border):
        d, ptr = self.d, self.lib.ptr
        self.status = self._out((self.n_edges,), torch.uint8, 249)
        self.keep, self.gone = self._out((self.n_edges,), torch.int64), self._out((self.n_edges,), torch.int64)
        d.sp_sd_hf_rm_status, d.sp_sd_hf_rm_keep, d.sp_sd_hf_rm_gone = ptr(self.status), ptr(self.keep), ptr(self.gone)
        d.sp_sd_hf_rm_low, d.sp_sd_hf_rm_high, d.sp_sd_hf_rm_cos_border = low, high, cos_border
        self.lib.call("nudf_meshremesh_collapse_check", d)
        return _host(self.status), _host(self.keep), _host(self.gone)

    def vertex_min(self, mode, rank, best_in=None):
        d, ptr = self.d, self.lib.ptr
        self.rank, self.best_in = _dev(rank), _dev(best_in)
        self.best = self._out((self.n_verts,), torch.int64)
        d.sp_sd_hf_rm_rank, d.sp_sd_hf_rm_mode = ptr(self.rank), mode
        d.sp_sd_hf_rm_best_in, d.sp_sd_hf_rm_best_out = ptr(self.best_in), ptr(self.best)
        self.lib.call("nudf_meshremesh_vertex_min", d)
        return _host(self.best)

    def collapse_apply(self, best):
        d, ptr = self.d, self.lib.ptr
        self.best_in = _dev(best)
        self.remap, self.pos_out = torch.arange(self.n_verts, dtype=torch.int64, device=DEV), self.pos.clone()
        self.win = self._out((self.n_edges,), torch.uint8, 249)
        d.sp_sd_hf_rm_best_in, d.sp_sd_hf_rm_remap, d.sp_sd_hf_rm_pos_out = ptr(self.best_in), ptr(self.remap), ptr(self.pos_out)
        d.sp_sd_hf_rm_win = ptr(self.win)
        self.lib.call("nudf_meshremesh_collapse_apply", d)
        return _host(self.remap), _host(self.pos_out), _host(self.win)

    def flip_check(self):
        d, ptr = self.d, self.lib.ptr
        self.status = self._out((self.n_edges,), torch.uint8, 249)
        self.gain, self.ab = self._out((self.n_edges,), torch.int32), self._out((self.n_edges, 2), torch.int64)
        d.sp_sd_hf_rm_status, d.sp_sd_hf_rm_gain, d.sp_sd_hf_rm_ab = ptr(self.status), ptr(self.gain), ptr(self.ab)
        self.lib.call("nudf_meshremesh_flip_check", d)
        return _host(self.status), _host(self.gain), _host(self.ab)

    def flip_apply(self, best):
        d, ptr = self.d, self.lib.ptr
        self.best_in, self.faces_out = _dev(best), self.faces.clone()
        self.win = self._out((self.n_edges,), torch.uint8, 249)
        d.sp_sd_hf_rm_best_in, d.sp_sd_hf_rm_faces_out, d.sp_sd_hf_rm_win = ptr(self.best_in), ptr(self.faces_out), ptr(self.win)
        self.lib.call("nudf_meshremesh_flip_apply", d)
        return _host(self.faces_out), _host(self.win)

    def relax(self):
        self.pos_out = torch.full((self.n_verts, 3), np.nan, dtype=torch.float64, device=DEV)
        self.d.sp_sd_hf_rm_pos_out = self.lib.ptr(self.pos_out)
        self.lib.call("nudf_meshremesh_relax", self.d)
        return _host(self.pos_out)


# ---- each entry point, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + tuple(EXTRA))
def test_tables_are_the_restatements(name):
    """what the restatement rebuilds of the driver's tables is what the kernels read"""
    v, f = MESHES[name]
    k, T = _Kernels(v, f), R.topo(f, len(v))
    e = _host(k.t.table.edges)
    np.testing.assert_array_equal(e, np.stack([T.table.u, T.table.v, T.table.count, T.face0, T.face1], 1))
    np.testing.assert_array_equal(_host(k.t.vclass), T.vclass)
    np.testing.assert_array_equal(_host(k.t.ring_off), T.ring_off)
    pos, faces, ring, boundary, corner_off, corner, vedge_off, vedge = k.t.held
    np.testing.assert_array_equal(_host(ring), T.ring)
    np.testing.assert_array_equal(_host(corner_off), T.corner_off)
    np.testing.assert_array_equal(_host(corner), T.corner)
    np.testing.assert_array_equal(_host(vedge_off), T.vedge_off)
    np.testing.assert_array_equal(_host(vedge), T.vedge)
    np.testing.assert_array_equal(_host(boundary.nbr), np.array([w for r in T.border for w in r], np.int64))


@pytest.mark.parametrize("name", NAMES + tuple(EXTRA))
def test_collapse_kernels_equal_the_restatement(name):
    v, f = MESHES[name]
    k, T = _Kernels(v, f), R.topo(f, len(v))
    seen = set()
    for factor, cos_border in [(x, COS30) for x in FACTORS] + [(1.5, 1.0), (2.25, -1.0)]:
        low, high = 0.8 * factor * MEAN[name], factor * MEAN[name] * 4 / 3
        status, keep, gone = R.collapse_check(v, f, T, low, high, cos_border)
        got = k.collapse_check(low, high, cos_border)
        np.testing.assert_array_equal(got[0], status)
        np.testing.assert_array_equal(got[1], keep)
        np.testing.assert_array_equal(got[2], gone)
        seen |= set(status.tolist())
        rank = R.ranks(status, R.edge_length2(v, T))
        best = None
        for mode in (0, 1, 1):
            want = R.vertex_min(T, f, status, rank, mode, best)
            np.testing.assert_array_equal(k.vertex_min(mode, rank, best), want)
            best = want
            remap, pos_out, win = R.collapse_apply(v, T, status, rank, keep, gone, best)      # after every pass: more winners
            got = k.collapse_apply(best)
            np.testing.assert_array_equal(got[0], remap)
            np.testing.assert_array_equal(got[1], pos_out)
            np.testing.assert_array_equal(got[2], win)
        assert win.sum() >= 1 or not (status == R.CANDIDATE).any()
    want = dict(sphere={R.CANDIDATE, R.LONG}, sheet={R.CANDIDATE, R.BORDER}, three={R.COUNT, R.CLASS}, awkward={R.COUNT, R.CLASS},
                cube={R.LINK, R.REACH}, jittered={R.FOLD, R.REACH}, dented={R.FOLD}, tetrahedron={R.DUPLICATE})
    assert seen >= want.get(name, set())


@pytest.mark.parametrize("name", NAMES + tuple(EXTRA))
def test_flip_kernels_equal_the_restatement(name):
    v, f = MESHES[name]
    k, T = _Kernels(v, f), R.topo(f, len(v))
    status, gain, ab = R.flip_check(v, f, T)
    got = k.flip_check()
    np.testing.assert_array_equal(got[0], status)
    np.testing.assert_array_equal(got[1], gain)
    np.testing.assert_array_equal(got[2], ab)
    rank = R.ranks(status, -gain.astype(np.int64))
    best = R.vertex_min(T, f, status, rank, 2)
    np.testing.assert_array_equal(k.vertex_min(2, rank), best)
    faces_out, win = R.flip_apply(f, T, status, rank, ab, best)
    got = k.flip_apply(best)
    np.testing.assert_array_equal(got[0], faces_out)
    np.testing.assert_array_equal(got[1], win)
    want = dict(cube={R.CANDIDATE, R.GAIN}, sheet={R.COUNT}, three={R.COUNT}, awkward={R.SAME, R.CLASS}, dented={R.FOLD},
                tetrahedron={R.EXISTS})
    assert set(status.tolist()) >= want.get(name, set())
    if name == "cube":
        assert win.sum() >= 1 and (faces_out != f).any(1).sum() == 2 * win.sum()


@pytest.mark.parametrize("name", NAMES + tuple(EXTRA))
def test_relax_equals_the_restatement(name):
    v, f = MESHES[name]
    want = R.relax(v, f, R.topo(f, len(v)))
    np.testing.assert_array_equal(_Kernels(v, f).relax(), want)
    if name in ("sphere", "cube", "jittered"):
        assert np.abs(want - v).max() > 1e-4


def test_out_of_range_table_entries_are_no_ops():
    """indices read from the tables that point outside them: nothing is written beyond the buffers, nothing wins"""
    v, f = MESHES["sheet"]
    k = _Kernels(v, f)
    low, high = 1.2 * MEAN["sheet"], 2.0 * MEAN["sheet"]
    status = k.collapse_check(low, high, COS30)[0]
    assert (status == R.CANDIDATE).any()
    rank = np.full(k.n_edges, 1 << 40, np.int64)                     # no rank is that large: "none"
    assert (k.vertex_min(0, rank) == k.n_edges).all() and (k.vertex_min(2, rank) == k.n_edges).all()
    rank = np.full(k.n_edges, -5, np.int64)
    assert (k.vertex_min(0, rank) == k.n_edges).all()
    best = np.zeros(len(v), np.int64)
    k.vertex_min(0, rank)
    assert k.collapse_apply(best)[2].sum() == 0
    k.flip_check()
    assert k.flip_apply(best)[1].sum() == 0
    ring = k.t.held[2]
    ring.fill_(1 << 33)                                                # every neighbour out of range
    assert (k.collapse_check(low, high, COS30)[0] != R.CANDIDATE).all()
    np.testing.assert_array_equal(k.relax(), v)
    assert (k.vertex_min(1, rank, best) == 0).all()


# ---- the driver, bit for bit -------------------------------------------------------------------------------------------------
def _same(got, want):
    assert got.verts.dtype == torch.from_numpy(want.verts[:0]).dtype
    np.testing.assert_array_equal(_host(got.verts), want.verts)
    np.testing.assert_array_equal(_host(got.faces), want.faces)
    assert (got.iterations, got.collapsed, got.flipped, got.split) == (want.iterations, want.collapsed, want.flipped, want.split)
    if want.attributes is None:
        assert got.attributes is None
    else:
        np.testing.assert_array_equal(_host(got.attributes), want.attributes)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name", NAMES)
def test_remesh_equals_the_restatement(name, factor):
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    target = factor * MEAN[name]
    got = meshing.remesh_isotropic(_dev(v), _dev(f), target, iterations=2, project=False)
    assert isinstance(got, meshing.Remeshed)
    _same(got, R.remesh_isotropic(v, f, target, iterations=2, project=False))


@pytest.mark.parametrize("name,factor,angle", [("sphere", 1.5, 30.0), ("sheet", 1.5, 0.0), ("squashed_ico2", 0.7, 90.0)])
def test_remesh_with_projection_equals_the_restatement(name, factor, angle):
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    attr = np.random.default_rng(len(v)).random((len(v), 3))
    target = factor * MEAN[name]
    got = meshing.remesh_isotropic(_dev(v), _dev(f), target, iterations=2, border_angle=angle, attributes=_dev(attr))
    want = R.remesh_isotropic(v, f, target, iterations=2, border_angle=angle, attributes=attr)
    _same(got, want)
    assert sum(want.collapsed) + sum(want.flipped) + sum(want.split) > 0
    if name == "sheet":                                                  # an angle of 0 keeps the border as it is
        assert R.border_edges(want.faces, len(want.verts)) == R.border_edges(f, len(v))


def test_float32_two_runs_and_nothing_to_do():
    from neuraludf_amd import meshing
    v, f = MESHES["squashed_ico2"]
    v32 = v.astype(np.float32)
    vt, ft = _dev(v32), _dev(f)
    info = {}
    a = meshing.remesh_isotropic(vt, ft, 0.25, iterations=3, _info=info)
    b = meshing.remesh_isotropic(vt, ft, 0.25, iterations=3)
    assert a.verts.dtype == torch.float32 and torch.equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and a[3:] == b[3:]
    _same(a, R.remesh_isotropic(v32, f, 0.25, iterations=3))
    assert len(info["rounds"]) == 3
    for it, log in enumerate(info["rounds"]):
        assert sum(r["winners"] for r in log["collapse"]) == a.collapsed[it]
        assert sum(r["winners"] for r in log["flip"]) == a.flipped[it]
        assert all(r["winners"] <= r["candidates"] for r in log["collapse"] + log["flip"])
    before, after = R.quality(v, f, 0.25), R.quality(_host(a.verts).astype(np.float64), _host(a.faces), 0.25)
    print(f"squashed_ico2 at L = 0.25, projected: share of edges in [0.8 L, 4/3 L] {before[0]:.3f} -> {after[0]:.3f}, "
          f"mean triangle quality {before[2]:.3f} -> {after[2]:.3f}")
    assert after[0] > before[0]
    ico, fi = MESHES["ico0"]
    same = meshing.remesh_isotropic(_dev(ico), _dev(fi), MEAN["ico0"], iterations=2)
    assert same.split == same.collapsed == same.flipped == (0, 0) and torch.equal(same.faces, _dev(fi))
    none = meshing.remesh_isotropic(vt, ft, 0.25, iterations=0)
    assert torch.equal(none.verts, vt) and torch.equal(none.faces, ft) and none[3:] == (0, (), (), ())
    capped = meshing.remesh_isotropic(vt, ft, 0.25, iterations=1, max_subrounds=0)
    assert capped.collapsed == capped.flipped == (0,) and capped.split[0] > 0
    empty = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    out = meshing.remesh_isotropic(vt, empty, 0.25)
    assert torch.equal(out.verts, vt) and out.faces.shape == (0, 3) and out.split == (0,) * 5


def test_the_winding_and_the_order_of_the_faces_change_nothing():
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    rng = np.random.default_rng(17)
    target = 1.5 * MEAN["sphere"]
    variants = [f[:, [0, 2, 1]], np.where((rng.random(len(f)) < 0.5)[:, None], f[:, [0, 2, 1]], f)]
    infos = [{} for _ in range(3)]
    base = meshing.remesh_isotropic(_dev(v), _dev(f), target, iterations=3, _info=infos[0])
    assert sum(base.split) > 0 and sum(base.collapsed) > 0 and sum(base.flipped) > 0
    want = {tuple(sorted(t)) for t in _host(base.faces).tolist()}
    for faces, info in zip(variants, infos[1:]):
        got = meshing.remesh_isotropic(_dev(v), _dev(np.ascontiguousarray(faces)), target, iterations=3, _info=info)
        assert got[3:] == base[3:] and info["rounds"] == infos[0]["rounds"]        # every sub-round's candidates and winners
        assert torch.equal(got.verts, base.verts)
        assert {tuple(sorted(t)) for t in _host(got.faces).tolist()} == want


def test_projected_vertices_lie_on_the_input_mesh():
    from neuraludf_amd import evaluation, meshing
    for name, target in (("sphere", 1.5 * MEAN["sphere"]), ("squashed_ico2", 0.25)):
        v, f = MESHES[name]
        vt, ft = _dev(v), _dev(f)
        diagonal = float(np.linalg.norm(v.max(0) - v.min(0)))
        out = meshing.remesh_isotropic(vt, ft, target, iterations=3)
        worst = float(evaluation.closest_on_mesh(out.verts, vt, ft).dist.max())
        print(f"{name}: largest distance of a remeshed vertex from the input mesh {worst:.3g} "
              f"({worst / diagonal:.3g} of the diagonal {diagonal:.3g})")
        assert worst <= 1e-12 * diagonal
        free = meshing.remesh_isotropic(vt, ft, target, iterations=3, project=False)
        assert float(evaluation.closest_on_mesh(free.verts, vt, ft).dist.max()) > 1e-4     # without it they leave the surface


def test_argument_errors():
    from neuraludf_amd import meshing
    v, f = MESHES["sheet"]
    vt, ft = _dev(v), _dev(f)
    for bad in (dict(target_edge=0.0), dict(target_edge=-1.0), dict(target_edge=float("nan")), dict(target_edge=float("inf")),
                dict(target_edge="long"), dict(target_edge=0.1, iterations=-1), dict(target_edge=0.1, iterations=1.5),
                dict(target_edge=0.1, max_subrounds=-1), dict(target_edge=0.1, border_angle=-1.0),
                dict(target_edge=0.1, border_angle=180.5), dict(target_edge=0.1, border_angle=float("nan")),
                dict(target_edge=0.1, attributes=torch.zeros((2, 3), dtype=torch.float64, device=DEV)),
                dict(target_edge=0.1, attributes=torch.zeros((len(v), 3), dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            meshing.remesh_isotropic(vt, ft, **bad)
    for a, b in ((vt.cpu(), ft.cpu()), (vt.half(), ft), (vt, ft.int()), (vt, ft + len(v))):
        with pytest.raises(ValueError):
            meshing.remesh_isotropic(a, b, 0.1)


# ---- wiring --------------------------------------------------------------------------------------------------------------
class _SphereUDF(torch.nn.Module):
    """| |x| - R | and its gradient behind the interface extract_udf_mesh queries (as in tests/test_gpu_meshsubdiv.py)"""

    def __init__(self, radius):
        super().__init__()
        self.radius = torch.nn.Parameter(torch.tensor(float(radius)), requires_grad=False)

    def udf(self, p):
        return (p.norm(dim=-1, keepdim=True) - self.radius).abs()

    def gradient(self, p):
        r = p.norm(dim=-1, keepdim=True)
        return torch.nan_to_num(p / r * torch.sign(r - self.radius))


def test_extract_udf_mesh_remeshes_after_it_simplifies():
    from neuraludf_amd import meshing
    udf = _SphereUDF(0.6).to(DEV)
    n = 33
    cell = 3.0 * meshing.grid_spacing(*BOX, n)
    v0, f0 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell)
    v1, f1 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell, remesh_edge=cell, remesh_iterations=2)
    want = meshing.remesh_isotropic(_dev(v0), _dev(f0), cell, iterations=2)
    np.testing.assert_array_equal(v1, _host(want.verts))
    np.testing.assert_array_equal(f1, _host(want.faces))
    assert sum(want.collapsed) + sum(want.flipped) > 0
    before = R.quality(v0.astype(np.float64), f0, cell)
    after = R.quality(v1.astype(np.float64), f1, cell)
    print(f"sphere UDF at {n}^3, cell {cell:.3g}: share of edges in [0.8 L, 4/3 L] {before[0]:.3f} -> {after[0]:.3f}, "
          f"smallest triangle quality {before[1]:.3f} -> {after[1]:.3f}, mean {before[2]:.3f} -> {after[2]:.3f}")
    assert after[0] > before[0]
    v2, f2 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell, remesh_edge=cell, remesh_iterations=2,
                                      orient=True)
    np.testing.assert_array_equal(v2, v1)
    assert R.consistently_wound(f2, len(v2)) and {tuple(sorted(t)) for t in f2.tolist()} == {tuple(sorted(t)) for t in f1.tolist()}


def test_cli_remeshes_and_carries_the_colours(tmp_path, capsys):
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    v32 = v.astype(np.float32)
    colours = np.random.default_rng(1).integers(40, 200, (len(v), 3)).astype(np.uint8)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    meshing.write_ply(src, v32, f, colors=colours)
    target = 1.5 * MEAN["sphere"]
    assert meshing.main([src, dst, "--remesh", repr(target), "--remesh-iterations", "2"]) == 0
    assert "remesh: split" in capsys.readouterr().out
    ov, of, oc = meshing.read_ply(dst, with_colors=True)
    rv, rf, rc = meshing.read_ply(src, with_colors=True)                       # in the reader's dtype, as the CLI holds it
    want = meshing.remesh_isotropic(_dev(rv), _dev(rf), target, iterations=2, attributes=_dev(rc.astype(np.float64)))
    np.testing.assert_array_equal(ov, _host(want.verts).astype(np.float32))
    np.testing.assert_array_equal(of, _host(want.faces))
    np.testing.assert_array_equal(oc, np.rint(np.clip(_host(want.attributes), 0.0, 255.0)).astype(np.uint8))
    assert oc.min() >= colours.min() and oc.max() <= colours.max()             # barycentric weights: no overshoot
    assert len(of) < len(f)
