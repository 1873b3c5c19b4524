"""GPU: mesh subdivision (neuraludf_amd/meshclean.py subdivide_mesh / subdivide_to_edge, csrc/meshsubdiv.hip) against the
numpy restatement (tests/meshsubdiv_ref.py), bit for bit: each entry point through the descriptor, then the two drivers --
plus the new vertices against the exact point-to-mesh distance, the mesher end to end and the CLI.

The distance cap.  A midpoint (p_u + p_v) 0.5 is one rounded sum per coordinate, exact halving: it lies within u |p| / 2 per
coordinate of the segment (u = 2^-52), and closest_on_mesh evaluates that segment in float64 as well, so the distance it
reports is a few u of the coordinates' size.  The issue holds it to 1e-12 of the bounding box's diagonal, four orders of
magnitude above that; the test prints what it measures."""
import numpy as np
import pytest
import torch

import meshsubdiv_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
RATIOS = (0.75, 0.3, 0.07)
MESH_NAMES = ("ico0", "fan", "three", "awkward", "sheet", "stretched", "sphere")


@pytest.fixture(scope="module", autouse=True)
def _hand_back_the_cache():
    """these tests leave float64 geometry in the blocks torch's allocator keeps; hand the blocks back, as
    tests/test_gpu_meshsmooth.py does"""
    yield
    torch.cuda.empty_cache()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


MESHES = {k: _frozen(*R.meshes()[k]) for k in MESH_NAMES}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # a copy: the fixtures' arrays are read-only


def _attr(v):
    """three attribute columns, the same for the kernel and the restatement"""
    return np.random.default_rng(len(v)).random((len(v), 3))


def _longest(v, f):
    return R.longest_edge(v, R.edge_table(f, len(v)))


@pytest.fixture(scope="module")
def want_to_edge():
    """the restatement's subdivide_to_edge with attributes, once per mesh and ratio"""
    out = {}
    for name, (v, f) in MESHES.items():
        for ratio in RATIOS:
            out[name, ratio] = R.subdivide_to_edge(v, f, ratio * _longest(v, f), attributes=_attr(v))
    return out


class _Kernels:
    """the five entry points on a mesh, through the descriptor, as the drivers call them"""

    def __init__(self, v, f, attr=None):
        from neuraludf_amd import _lib, meshclean
        self.lib, self.n_verts, self.n_faces = _lib, len(v), len(f)
        self.pos, self.faces, self.attr = _dev(v), _dev(f), _dev(attr)
        self.table = meshclean._mesh_edges(self.faces, len(v))
        self.d = meshclean._topo(self.faces, len(v), self.table)
        self.d.pos = _lib.ptr(self.pos)
        if attr is not None:
            self.d.sp_attr, self.d.sp_attr_width = _lib.ptr(self.attr), attr.shape[1]

    def mark(self, max_edge=None):
        out = torch.empty(self.table.edges.shape[0], dtype=torch.uint8, device=DEV)
        self.d.sp_sd_mark, self.d.sp_sd_mark_all = self.lib.ptr(out), int(max_edge is None)
        self.d.sp_sd_max_edge = 0.0 if max_edge is None else max_edge
        self.lib.call("nudf_meshsubdiv_mark", self.d)
        return out.cpu().numpy().astype(bool)

    def vertices(self, marks, scheme):
        """odd and even -> (positions, attributes or None) of the old and the new vertices"""
        from neuraludf_amd import meshclean
        self.marked = _dev(np.nonzero(marks)[0].astype(np.int64))
        n = self.n_verts + self.marked.numel()
        self.pos_out = torch.full((n, 3), np.nan, dtype=torch.float64, device=DEV)
        attr_out = None if self.attr is None else torch.full((n, self.attr.shape[1]), np.nan, dtype=torch.float64, device=DEV)
        d, ptr = self.d, self.lib.ptr
        d.sp_sd_marked, d.sp_sd_n_marked, d.sp_sd_scheme = ptr(self.marked), self.marked.numel(), R.SCHEMES.index(scheme)
        d.sp_sd_pos_out, d.sp_sd_attr_out = ptr(self.pos_out), ptr(attr_out)
        if scheme == "loop":
            self.ring_off, self.ring = meshclean._vertex_adjacency(self.faces, self.n_verts, self.table)
            self.border = meshclean._boundary(self.table, self.n_verts)
            self.vclass = meshclean._loop_classes(self.table, self.border, self.n_verts)
            d.sp_sd_ring_off, d.sp_sd_ring, d.sp_sd_n_ring = ptr(self.ring_off), ptr(self.ring), self.ring.numel()
            d.nbr_off, d.nbr, d.sp_sd_n_border = ptr(self.border.nbr_off), ptr(self.border.nbr), self.border.nbr.numel()
            d.sp_sd_vclass = ptr(self.vclass)
        self.lib.call("nudf_meshsubdiv_odd", d)
        self.lib.call("nudf_meshsubdiv_even", d)
        return self.pos_out.cpu().numpy(), None if attr_out is None else attr_out.cpu().numpy()

    def faces_of(self, marks):
        """count and emit, after vertices() -> (counts, faces', parent)"""
        d, ptr = self.d, self.lib.ptr
        edge_vertex = _dev(R.edge_vertices(marks, self.n_verts))
        fcount = torch.empty(self.n_faces, dtype=torch.int64, device=DEV)
        d.sp_sd_edge_vertex, d.sp_sd_fcount = ptr(edge_vertex), ptr(fcount)
        self.lib.call("nudf_meshsubdiv_count", d)
        foff = torch.cumsum(fcount, 0) - fcount
        n_out = int(fcount.sum())
        out = torch.full((n_out, 3), -7, dtype=torch.int64, device=DEV)
        parent = torch.full((n_out,), -7, dtype=torch.int64, device=DEV)
        d.sp_sd_foff, d.sp_sd_faces_out, d.sp_sd_parent, d.sp_sd_n_out = ptr(foff), ptr(out), ptr(parent), n_out
        self.lib.call("nudf_meshsubdiv_emit", d)
        return fcount.cpu().numpy(), out.cpu().numpy(), parent.cpu().numpy()


def _same(got, want):
    assert got.verts.dtype == torch.from_numpy(want.verts[:0]).dtype
    np.testing.assert_array_equal(got.verts.cpu().numpy(), want.verts)
    np.testing.assert_array_equal(got.faces.cpu().numpy(), want.faces)
    np.testing.assert_array_equal(got.parent_face.cpu().numpy(), want.parent_face)
    if want.attributes is None:
        assert got.attributes is None
    else:
        np.testing.assert_array_equal(got.attributes.cpu().numpy(), want.attributes)
    assert (got.rounds, got.longest_edge, got.converged) == (want.rounds, want.longest_edge, want.converged)


# ---- each entry point, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESH_NAMES)
def test_edge_table_is_the_restatements(name):
    """what the restatement rebuilds of the EdgeTable is what the kernels read"""
    v, f = MESHES[name]
    k, t = _Kernels(v, f), R.edge_table(f, len(v))
    e = k.table.edges.cpu().numpy()
    np.testing.assert_array_equal(e[:, :3], np.stack([t.u, t.v, t.count], 1))
    np.testing.assert_array_equal(k.table.he_edge.cpu().numpy(), t.he_edge)
    np.testing.assert_array_equal(k.table.he_id.cpu().numpy(), t.he_id)
    np.testing.assert_array_equal(k.table.edge_start.cpu().numpy(), t.edge_start)


@pytest.mark.parametrize("name", MESH_NAMES)
def test_mark_equals_the_restatement(name):
    v, f = MESHES[name]
    k, t = _Kernels(v, f), R.edge_table(f, len(v))
    np.testing.assert_array_equal(k.mark(), R.mark(v, t))
    assert k.mark().sum() == (t.u != t.v).sum()
    bound = 0.3 * _longest(v, f)
    want = R.mark(v, t, bound)
    np.testing.assert_array_equal(k.mark(bound), want)
    assert want.any()                                # (some but not all: the stretched sheet of the next test)
    # the rounded length of the median edge as the bound (an edge of exactly the bound: the next test)
    d2 = R._dist2(v[t.u], v[t.v])
    bound = float(np.sqrt(np.sort(d2[t.u != t.v])[(t.u != t.v).sum() // 2]))
    np.testing.assert_array_equal(k.mark(bound), R.mark(v, t, bound))


def test_mark_leaves_out_an_edge_of_exactly_the_bound():
    v, f = MESHES["stretched"]                       # spacings 12.5 and 0.25: the squares are exact
    k, t = _Kernels(v, f), R.edge_table(f, len(v))
    d2 = R._dist2(v[t.u], v[t.v])
    assert (d2 == 156.25).any() and (d2 > 156.25).any()
    got = k.mark(12.5)
    np.testing.assert_array_equal(got, d2 > 156.25)
    assert not got[d2 == 156.25].any() and got.any()
    nan = np.array(v)
    nan[0, 0] = np.nan
    got = _Kernels(nan, f).mark(0.1)
    np.testing.assert_array_equal(got, R.mark(nan, t, 0.1))
    assert not got[(t.u == 0) | (t.v == 0)].any()   # a NaN length is not marked


@pytest.mark.parametrize("width", [0, 3])
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("name", MESH_NAMES)
def test_vertices_equal_the_restatement(name, scheme, width):
    """odd and even, with every edge marked and with the long ones only"""
    v, f = MESHES[name]
    attr = _attr(v) if width else None
    k, t = _Kernels(v, f, attr), R.edge_table(f, len(v))
    for marks in (R.mark(v, t), R.mark(v, t, 0.3 * _longest(v, f))):
        pos, att = k.vertices(marks, scheme)
        np.testing.assert_array_equal(pos, np.concatenate([R.even(v, f, t, scheme), R.odd(v, f, t, marks, scheme)]))
        if width:
            np.testing.assert_array_equal(att, np.concatenate([R.even(attr, f, t, scheme), R.odd(attr, f, t, marks, scheme)]))
        else:
            assert att is None
    if scheme == "loop":
        np.testing.assert_array_equal(k.vclass.cpu().numpy(), R.vertex_classes(t, len(v)))
        assert np.abs(pos[:len(v)] - v).max() > 1e-4
    else:
        np.testing.assert_array_equal(pos[:len(v)], v)


@pytest.mark.parametrize("name", MESH_NAMES)
def test_count_and_emit_equal_the_restatement(name):
    v, f = MESHES[name]
    k, t = _Kernels(v, f), R.edge_table(f, len(v))
    rng = np.random.default_rng(7)
    proper = t.u != t.v
    for marks in (R.mark(v, t), R.mark(v, t, 0.3 * _longest(v, f)), proper & (rng.random(len(proper)) < 0.5)):
        pos, _ = k.vertices(marks, "midpoint")
        ev = R.edge_vertices(marks, len(v))
        fcount, faces, parent = k.faces_of(marks)
        np.testing.assert_array_equal(fcount, R.count(t, ev, len(f)))
        want_faces, want_parent = R.emit(f, t, ev, pos)
        np.testing.assert_array_equal(faces, want_faces)
        np.testing.assert_array_equal(parent, want_parent)
        assert faces.min() >= 0 and faces.max() < len(pos)


# ---- the drivers, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("name", MESH_NAMES)
def test_subdivide_mesh_equals_the_restatement(name, scheme):
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    attr = _attr(v)
    for levels in (1, 2):
        got = meshing.subdivide_mesh(_dev(v), _dev(f), levels, scheme, attributes=_dev(attr))
        assert isinstance(got, meshing.Subdivided) and got.rounds == levels and got.converged
        _same(got, R.subdivide_mesh(v, f, levels, scheme, attributes=attr))
    _same(meshing.subdivide_mesh(_dev(v), _dev(f), 1, scheme), R.subdivide_mesh(v, f, 1, scheme))
    zero = meshing.subdivide_mesh(_dev(v), _dev(f), 0, scheme)
    _same(zero, R.subdivide_mesh(v, f, 0, scheme))
    assert zero.rounds == 0 and zero.longest_edge == _longest(v, f)


@pytest.mark.parametrize("name", MESH_NAMES)
def test_subdivide_to_edge_equals_the_restatement(name, want_to_edge):
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    L = _longest(v, f)
    for ratio in RATIOS:
        want = want_to_edge[name, ratio]
        got = meshing.subdivide_to_edge(_dev(v), _dev(f), ratio * L, attributes=_dev(_attr(v)))
        _same(got, want)
        assert got.converged and got.longest_edge <= ratio * L and got.rounds == R.expected_rounds(L, ratio * L)
    got = meshing.subdivide_to_edge(_dev(v), _dev(f), 0.07 * L, max_rounds=2)
    _same(got, R.subdivide_to_edge(v, f, 0.07 * L, max_rounds=2))
    assert not got.converged and got.rounds == 2 and got.longest_edge > 0.07 * L
    none = meshing.subdivide_to_edge(_dev(v), _dev(f), 0.07 * L, max_rounds=0)
    assert not none.converged and none.rounds == 0 and torch.equal(none.faces, _dev(f)) and none.longest_edge == L


def test_float32_in_float32_out():
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    v32, a32 = v.astype(np.float32), _attr(v).astype(np.float32)
    for scheme in R.SCHEMES:
        got = meshing.subdivide_mesh(_dev(v32), _dev(f), 2, scheme, attributes=_dev(a32))
        assert got.verts.dtype == got.attributes.dtype == torch.float32
        _same(got, R.subdivide_mesh(v32, f, 2, scheme, attributes=a32))     # float64 on the upcast input, cast at the end
    bound = 0.3 * _longest(v32.astype(np.float64), f)
    got = meshing.subdivide_to_edge(_dev(v32), _dev(f), bound, attributes=_dev(a32))
    assert got.verts.dtype == got.attributes.dtype == torch.float32
    _same(got, R.subdivide_to_edge(v32, f, bound, attributes=a32))


def test_two_runs_and_nothing_to_do():
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    vt, ft = _dev(v), _dev(f)
    runs = [lambda: meshing.subdivide_mesh(vt, ft, 2, "loop"), lambda: meshing.subdivide_mesh(vt, ft, 2, "midpoint"),
            lambda: meshing.subdivide_to_edge(vt, ft, 0.07 * _longest(v, f))]
    for run in runs:
        a, b = run(), run()
        assert torch.equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and torch.equal(a.parent_face, b.parent_face)
        assert a[4:] == b[4:]
    empty = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    for out in (meshing.subdivide_mesh(vt, empty), meshing.subdivide_to_edge(vt, empty, 0.1)):
        assert torch.equal(out.verts, vt) and out.faces.shape == (0, 3) and out.parent_face.shape == (0,)
        assert out.rounds == 0 and out.converged and out.longest_edge == 0.0
    out = meshing.subdivide_mesh(vt[:0], empty, attributes=vt[:0])
    assert out.verts.shape == (0, 3) and out.attributes.shape == (0, 3)


def test_argument_errors():
    from neuraludf_amd import meshing
    v, f = MESHES["three"]
    vt, ft = _dev(v), _dev(f)
    for bad in (dict(levels=-1), dict(levels=1.5), dict(levels="two"), dict(scheme="butterfly"), dict(scheme=None),
                dict(attributes=torch.zeros((len(v) + 1, 3), dtype=torch.float64, device=DEV)),
                dict(attributes=torch.zeros(len(v), dtype=torch.float64, device=DEV)),
                dict(attributes=torch.zeros((len(v), 3), dtype=torch.int64, device=DEV)),
                dict(attributes=torch.zeros((len(v), 3), dtype=torch.float64))):
        with pytest.raises(ValueError):
            meshing.subdivide_mesh(vt, ft, **bad)
    for bad in (dict(max_edge=0.0), dict(max_edge=-1.0), dict(max_edge=float("nan")), dict(max_edge=float("inf")),
                dict(max_edge="long"), dict(max_edge=0.5, max_rounds=-1), dict(max_edge=0.5, max_rounds=2.5),
                dict(max_edge=0.5, attributes=torch.zeros((2, 3), dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            meshing.subdivide_to_edge(vt, ft, **bad)
    for call in (lambda a, b: meshing.subdivide_mesh(a, b), lambda a, b: meshing.subdivide_to_edge(a, b, 0.5)):
        with pytest.raises(ValueError):
            call(vt.cpu(), ft.cpu())
        with pytest.raises(ValueError):
            call(vt.half(), ft)
        with pytest.raises(ValueError):
            call(vt, ft.int())
        with pytest.raises(ValueError):
            call(vt, ft + len(v))


# ---- against the distance code -------------------------------------------------------------------------------------------------
def test_split_vertices_lie_on_the_input_mesh():
    from neuraludf_amd import evaluation, meshing
    v, f = MESHES["sphere"]
    vt, ft = _dev(v), _dev(f)
    diagonal = float(np.linalg.norm(v.max(0) - v.min(0)))
    worst = 0.0
    for out in (meshing.subdivide_mesh(vt, ft, 2, "midpoint"), meshing.subdivide_to_edge(vt, ft, 0.3 * _longest(v, f))):
        c = evaluation.closest_on_mesh(out.verts, vt, ft)
        worst = max(worst, float(c.dist.max()))
        assert float(c.dist[:len(v)].max()) == 0.0                             # the old vertices are the mesh's own
    print(f"noisy_sphere: largest distance of a midpoint vertex from the input mesh {worst:.3g} "
          f"({worst / diagonal:.3g} of the diagonal {diagonal:.3g})")
    assert worst <= 1e-12 * diagonal
    loop = meshing.subdivide_mesh(vt, ft, 1, "loop")
    assert float(evaluation.closest_on_mesh(loop.verts, vt, ft).dist.max()) > 1e-4    # Loop leaves the surface


# ---- wiring --------------------------------------------------------------------------------------------------------------
class _SphereUDF(torch.nn.Module):
    """| |x| - R | and its gradient behind the interface extract_udf_mesh queries"""

    def __init__(self, radius):
        super().__init__()
        self.radius = torch.nn.Parameter(torch.tensor(float(radius)), requires_grad=False)

    def udf(self, p):
        return (p.norm(dim=-1, keepdim=True) - self.radius).abs()

    def gradient(self, p):
        r = p.norm(dim=-1, keepdim=True)
        return torch.nan_to_num(p / r * torch.sign(r - self.radius))


def _max_edge(v, f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return float(np.linalg.norm(v[e[:, 0]].astype(np.float64) - v[e[:, 1]].astype(np.float64), axis=1).max())


def test_extract_udf_mesh_subdivides_before_it_colours():
    import meshraster_scenes
    from neuraludf_amd import meshing
    udf = _SphereUDF(0.6).to(DEV)
    n = 33
    cell = 3.0 * meshing.grid_spacing(*BOX, n)
    h = 0.4 * cell
    mats = meshraster_scenes.pinhole(40.0, 32.0, 24.0, C=(0.0, 0.0, -2.0))[None]
    imgs = torch.full((1, 48, 64, 3), 0.625, dtype=torch.float32, device=DEV)
    v0, f0 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell)
    v1, f1, c1 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell, subdivide_max_edge=h,
                                          color_from=(mats, imgs))
    want = meshing.subdivide_to_edge(_dev(v0), _dev(f0), h)
    np.testing.assert_array_equal(v1, want.verts.cpu().numpy())
    np.testing.assert_array_equal(f1, want.faces.cpu().numpy())
    assert _max_edge(v0, f0) > h and len(v1) > len(v0)
    # the vertices come back as float32: inside the box a coordinate moves by at most 2^-25, an end by sqrt(3) times that
    assert _max_edge(v1, f1) <= h + 2.0 * np.sqrt(3.0) * 2.0 ** -25
    assert want.converged and want.longest_edge <= h
    assert c1.shape == (len(v1), 3) and c1.dtype == np.float32 and (c1 == np.float32(0.625)).all(1).any()
    v2, f2 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell, subdivide_max_edge=h, subdivide=1)
    both = meshing.subdivide_mesh(want.verts, want.faces, 1, "loop")
    np.testing.assert_array_equal(v2, both.verts.cpu().numpy())
    np.testing.assert_array_equal(f2, both.faces.cpu().numpy())
    v3, f3 = meshing.extract_udf_mesh(udf, n, keep_largest=True, simplify_cell=cell, subdivide=dict(levels=1, scheme="midpoint"))
    np.testing.assert_array_equal(v3, meshing.subdivide_mesh(_dev(v0), _dev(f0), 1, "midpoint").verts.cpu().numpy())
    assert len(f3) == 4 * len(f0)


def test_cli_round_trip_subdivides_and_carries_the_colours(tmp_path, capsys):
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    v32 = v.astype(np.float32)
    colours = np.random.default_rng(1).integers(40, 200, (len(v), 3)).astype(np.uint8)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    meshing.write_ply(src, v32, f, colors=colours)
    cell, h = 0.25, 0.2
    assert meshing.main([src, dst, "--simplify", str(cell), "--max-edge", str(h), "--subdivide", "1",
                         "--subdivide-scheme", "loop"]) == 0
    ov, of, oc = meshing.read_ply(dst, with_colors=True)
    rv, rf, rc = meshing.read_ply(src, with_colors=True)                       # in the reader's dtype, as the CLI holds it
    s = meshing.simplify_mesh(_dev(rv), _dev(rf), cell, attributes=_dev(rc.astype(np.float64)))
    carried = torch.from_numpy(np.rint(s.attributes.cpu().numpy()).astype(np.uint8).astype(np.float64)).to(DEV)
    e = meshing.subdivide_to_edge(s.verts, s.faces, h, attributes=carried)
    n_edges = R.euler(e.verts.cpu().numpy(), e.faces.cpu().numpy())[1]
    u = meshing.subdivide_mesh(e.verts, e.faces, 1, "loop", attributes=e.attributes)
    assert e.rounds >= 1 and len(ov) == e.verts.shape[0] + n_edges == u.verts.shape[0] and len(of) == 4 * e.faces.shape[0]
    np.testing.assert_array_equal(ov, u.verts.cpu().numpy().astype(np.float32))  # the file holds float32
    np.testing.assert_array_equal(of, u.faces.cpu().numpy())
    assert oc is not None and oc.shape == (len(ov), 3) and oc.dtype == np.uint8
    np.testing.assert_array_equal(oc, np.rint(u.attributes.cpu().numpy()).astype(np.uint8))
    unit = oc.astype(np.float64) / 255.0
    assert unit.min() >= 0.0 and unit.max() <= 1.0
    assert oc.min() >= colours.min() and oc.max() <= colours.max()             # every weight is positive: no overshoot
    # without a simplification the file's own colours travel
    assert meshing.main([src, dst, "--subdivide", "1", "--subdivide-scheme", "midpoint"]) == 0
    ov, of, oc = meshing.read_ply(dst, with_colors=True)
    want = R.subdivide_mesh(rv, rf, 1, "midpoint", attributes=rc.astype(np.float64))
    np.testing.assert_array_equal(ov, want.verts.astype(np.float32))
    np.testing.assert_array_equal(oc[:len(v)], colours)
    np.testing.assert_array_equal(oc, np.rint(want.attributes).astype(np.uint8))
    with pytest.raises(SystemExit):
        meshing.main([src, dst, "--subdivide-scheme", "butterfly"])
