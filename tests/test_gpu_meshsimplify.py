"""GPU: the mesh simplification (neuraludf_amd/meshclean.py simplify_mesh / simplify_to_faces, csrc/meshsimplify.hip)
against the numpy restatement (tests/meshsimplify_ref.py): faces, vertex_cluster, face_src and accepted bit for bit,
positions, quadrics and attribute means to 1e-9 cell -- plus the key arithmetic near 2^60, the degenerate grids, the face
target, the mesher end to end, the CLI and the argument checks.

Why the accept decisions may be asked to match exactly: kernel and restatement add the same terms in the same order, the
solve's condition is at most (1 + lambda) / lambda = 1001, so a Cholesky factorisation in float64 is good to about 1e-12
relative, and tests/test_meshsimplify_ref.py shows that no solution of these inputs lies within 1e-6 cell of a wall."""
import numpy as np
import pytest
import torch

import meshorient_ref as O
import meshsimplify_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
TOL = 1e-9                                  # times the cell: positions, quadric entries and attribute means


@pytest.fixture(scope="module", autouse=True)
def _hand_back_the_cache():
    """these tests leave float64 geometry in the blocks torch's allocator keeps; buffers that later tests take from it
    with torch.empty would start with those bits in their pad rows.  Hand the blocks back."""
    yield
    torch.cuda.empty_cache()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cases' arrays are read-only


def _assert_matches(got, info, want, cell, float32_ulp=0.0):
    """got: Simplified of device tensors and its _info; want: the restatement's.  float32_ulp: for float32 vertices, one
    float32 ulp at the largest coordinate -- the two float64 results may lie on either side of a rounding boundary"""
    from neuraludf_amd import meshing
    assert isinstance(got, meshing.Simplified)
    for name in ("faces", "vertex_cluster", "face_src", "accepted"):
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)
    v = got.verts.cpu().numpy()
    assert v.dtype == want.verts.dtype and v.shape == want.verts.shape
    err = np.abs(v.astype(np.float64) - want.verts.astype(np.float64)).max()
    q = info["quadric"].cpu().numpy()
    assert q.shape == want.quadric.shape == (len(v), 10)
    qerr = np.abs(q - want.quadric).max()
    print(f"positions {err / cell:.3g} cell, quadrics {qerr / cell:.3g} cell")
    assert err <= TOL * cell + float32_ulp and qerr <= TOL * cell
    assert info["clusters"] == want.clusters and list(info["grid"]) == want.grid.tolist()
    if want.attributes is None:
        assert got.attributes is None
    else:
        a = got.attributes.cpu().numpy()
        assert a.dtype == want.attributes.dtype and a.shape == want.attributes.shape
        assert np.abs(a - want.attributes).max() <= TOL * cell


@pytest.fixture(scope="module")
def wanted():
    """the restatement's answers for the shared cases, computed once"""
    return {name: S.simplify(c["v"], c["f"], c["cell"], origin=c["origin"], attributes=c["attributes"])
            for name, c in S.cases().items()}


@pytest.mark.parametrize("name", list(S.cases()))
def test_equals_the_restatement(name, wanted):
    """fold, flat, sphere, mixed (closed + open + Moebius band + three faces on an edge + a repeated vertex + unused
    vertices) and fan: one cluster of 300 corners among ordinary ones"""
    from neuraludf_amd import meshing
    case, want = S.cases()[name], wanted[name]
    args = (_dev(case["v"]), _dev(case["f"]), case["cell"])
    kw = dict(origin=None if case["origin"] is None else tuple(case["origin"]), attributes=_dev(case["attributes"]))
    info = {}
    got = meshing.simplify_mesh(*args, _info=info, **kw)
    print(f"{name}: {len(case['f'])} -> {got.faces.shape[0]} faces, {info['clusters']} clusters, {info['fallbacks']} at the mean")
    assert 0 < got.faces.shape[0] < len(case["f"]) and info["fallbacks"] == int((~want.accepted).sum())
    _assert_matches(got, info, want, case["cell"])
    again = meshing.simplify_mesh(*args, **kw)                       # no _info: the quadric is not stored
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,kw", [("fold", dict(placement="mean")), ("flat", dict(boundary_weight=0.0)),
                                     ("mixed", dict(boundary_weight=2.5, regularisation=1e-2))])
def test_the_other_settings_equal_the_restatement(name, kw):
    from neuraludf_amd import meshing
    case = S.cases()[name]
    want = S.simplify(case["v"], case["f"], case["cell"], origin=case["origin"], **kw)
    assert want.wall_margin > 1e-6
    info = {}
    got = meshing.simplify_mesh(_dev(case["v"]), _dev(case["f"]), case["cell"], origin=case["origin"], _info=info, **kw)
    _assert_matches(got, info, want, case["cell"])
    if kw.get("placement") == "mean":
        assert not bool(got.accepted.any()) and info["fallbacks"] == 0 and not bool(info["quadric"].any())


def test_float32_vertices_give_float32_vertices():
    from neuraludf_amd import meshing
    case = S.cases()["sphere"]
    v32, a32 = case["v"].astype(np.float32), case["attributes"].astype(np.float32)
    want = S.simplify(v32, case["f"], case["cell"], attributes=a32)
    assert want.wall_margin > 1e-6 and want.verts.dtype == np.float32
    info = {}
    got = meshing.simplify_mesh(_dev(v32), _dev(case["f"]), case["cell"], attributes=_dev(a32), _info=info)
    assert got.verts.dtype == torch.float32 and got.attributes.dtype == torch.float32
    # the attribute means are float64 means rounded to float32: one float32 ulp at 1
    assert np.abs(got.attributes.cpu().numpy().astype(np.float64) - want.attributes).max() <= 2.0 ** -23
    got = got._replace(attributes=None)
    _assert_matches(got, info, want._replace(attributes=None), case["cell"], 2.0 ** -23 * float(np.abs(v32).max()))


def test_keys_near_2_to_the_60_are_exact():
    """grid dimensions 2^20 - 1 on every axis: an int32 or a float32 anywhere in the key path merges or splits clusters"""
    from neuraludf_amd import meshing
    v, f, cell, origin = S.key_patch()
    want = S.simplify(v, f, cell, origin=origin)
    info = {}
    got = meshing.simplify_mesh(_dev(v), _dev(f), cell, origin=tuple(origin), _info=info)
    assert list(info["grid"]) == [S.MAX_GRID - 1] * 3 and 0 < got.faces.shape[0] < 200
    _assert_matches(got, info, want, cell)
    with pytest.raises(ValueError, match="2\\^20"):
        meshing.simplify_mesh(_dev(v), _dev(f), cell, origin=tuple(origin - 2.0 * cell))


def test_one_cluster_for_the_whole_mesh():
    from neuraludf_amd import meshing
    case = S.cases()["sphere"]
    info = {}
    got = meshing.simplify_mesh(_dev(case["v"]), _dev(case["f"]), 5.0, attributes=_dev(case["attributes"]), _info=info)
    assert info["clusters"] == 1 and info["grid"] == [1, 1, 1]
    assert got.verts.shape == (0, 3) and got.faces.shape == (0, 3) and got.attributes.shape == (0, 3)
    assert got.face_src.shape == (0,) and got.accepted.shape == (0,) and bool((got.vertex_cluster == -1).all())


def test_simplify_to_faces():
    from neuraludf_amd import meshing
    case = S.cases()["sphere"]
    v, f = _dev(case["v"]), _dev(case["f"])
    for target in (1000, 200, 20):
        got = meshing.simplify_to_faces(v, f, target)
        want = S.simplify_to_faces(case["v"], case["f"], target)
        print(f"target {target}: {got.faces.shape[0]} faces")
        assert 0 < got.faces.shape[0] <= target
        np.testing.assert_array_equal(got.faces.cpu().numpy(), want.faces)
        np.testing.assert_array_equal(got.face_src.cpu().numpy(), want.face_src)
    for target in (len(case["f"]), len(case["f"]) + 7):
        got = meshing.simplify_to_faces(v, f, target, attributes=_dev(case["attributes"]))
        assert torch.equal(got.verts, v) and torch.equal(got.faces, f) and not bool(got.accepted.any())
        assert got.vertex_cluster.tolist() == list(range(len(case["v"]))) and got.face_src.tolist() == list(range(len(f)))
        assert torch.equal(got.attributes, _dev(case["attributes"]))
    got = meshing.simplify_to_faces(v, f, 0)
    assert got.faces.shape == (0, 3) and got.verts.shape == (0, 3)
    for bad in (-1, 2.5, "many", None):
        with pytest.raises(ValueError):
            meshing.simplify_to_faces(v, f, bad)
    with pytest.raises(ValueError):
        meshing.simplify_to_faces(v, f, 100, cell=0.1)


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


def test_extract_udf_mesh_simplifies_before_it_orients():
    from neuraludf_amd import evaluation, meshing
    udf = _SphereUDF(0.6).to(DEV)
    n = 33
    cell = 2.0 * meshing.grid_spacing(*BOX, n)
    v0, f0 = meshing.extract_udf_mesh(udf, n, orient=True)
    v1, f1 = meshing.extract_udf_mesh(udf, n, orient=True, simplify_cell=cell)
    print(f"N = {n}: {len(f0)} -> {len(f1)} faces")
    assert 0 < len(f1) < len(f0) and len(v1) < len(v0) and v1.dtype == np.float32 and f1.dtype == np.int64
    got = meshing.orient_faces(_dev(v1), _dev(f1))                    # already oriented: nothing left to flip
    assert not bool(got.flipped.any()) and bool(got.orientable.any())
    assert O.incompatible_edges(f1, got.orientable.cpu().numpy()) == 0
    assert bool(torch.isfinite(meshing.vertex_normals(_dev(v1), _dev(f1))).all())
    # every vertex of the full mesh has its cluster's vertex within the cell's diagonal, and that vertex is on the mesh
    dense = evaluation.sample_mesh(_dev(v1), _dev(f1), 0.25 * cell)
    dist, _ = evaluation.nearest(_dev(v0).double(), dense)
    back, _ = evaluation.nearest(_dev(v1).double(), _dev(v0).double())
    print(f"full -> simplified {float(dist.max()) / cell:.3f} cell, simplified -> full {float(back.max()) / cell:.3f} cell")
    assert float(dist.max()) <= np.sqrt(3.0) * cell and float(back.max()) <= np.sqrt(3.0) * cell


def test_cli_round_trip_with_colours(tmp_path, capsys):
    from neuraludf_amd import meshing
    case = S.cases()["sphere"]
    v, f, cell = case["v"].astype(np.float32), case["f"], case["cell"]
    colours = np.rint(case["attributes"] * 255.0).astype(np.uint8)
    meshing.write_ply(tmp_path / "in.ply", v, f, colors=colours)
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--simplify", str(cell), "--orient"]) == 0
    out = capsys.readouterr().out
    want = S.simplify(v.astype(np.float64), f, cell, attributes=colours.astype(np.float64))
    assert want.wall_margin > 1e-6
    assert f"simplify: {want.clusters} clusters, {int((~want.accepted).sum())} of {len(want.verts)} vertices at the mean" in out
    assert out.index("simplify:") < out.index("orient:")                            # the orientation sees the final mesh
    ov, of, oc = meshing.read_ply(tmp_path / "out.ply", with_colors=True)
    np.testing.assert_array_equal(np.sort(of, 1), np.sort(want.faces, 1))          # --orient may flip faces
    assert O.incompatible_edges(of) == 0
    assert np.abs(ov - want.verts).max() <= TOL * cell + 2.0 ** -23 * float(np.abs(v).max())       # written as float32
    # the means of 0..255 values, rounded to the nearest: off by one only where a mean lies within 1e-9 of a half
    means = want.attributes
    assert oc.dtype == np.uint8 and oc.shape == means.shape
    clear = np.abs(means - np.floor(means) - 0.5) > 1e-9
    np.testing.assert_array_equal(oc[clear], np.rint(means[clear]).astype(np.uint8))
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "to.ply"), "--simplify-to", "100"]) == 0
    tv, tf, tc = meshing.read_ply(tmp_path / "to.ply", with_colors=True)
    assert 0 < len(tf) <= 100 and tc.shape == (len(tv), 3) and tf.max() == len(tv) - 1
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "same.ply")]) == 0     # no switch: as before
    sv, sf, sc = meshing.read_ply(tmp_path / "same.ply", with_colors=True)
    assert len(sf) == len(f) and sc is None
    with pytest.raises(SystemExit):
        meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "x.ply"), "--simplify", "0.1", "--simplify-to", "10"])


def test_argument_errors_and_empty_meshes():
    from neuraludf_amd import meshing
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.5]], device=DEV)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], device=DEV)
    for bad_v, bad_f in [(v, f.int()), (v, f.cpu()), (v.cpu(), f), (v, f[:, :2]), (v[:, :2], f), (v.half(), f), (v[:3], f),
                         (v, f - 1), (v.cpu().numpy(), f), (v, f.cpu().numpy())]:
        with pytest.raises(ValueError):
            meshing.simplify_mesh(bad_v, bad_f, 0.5)
        with pytest.raises(ValueError):
            meshing.simplify_to_faces(bad_v, bad_f, 1)
    for cell in (0.0, -1.0, float("nan"), float("inf"), "wide", None, 1e-7):
        with pytest.raises(ValueError):
            meshing.simplify_mesh(v, f, cell)
    for kw in (dict(origin=(0.0, 0.0)), dict(origin=(0.0, float("nan"), 0.0)), dict(origin="abc"),
               dict(origin=(0.5, 0.0, 0.0)), dict(placement="median"), dict(boundary_weight=-1.0),
               dict(boundary_weight=float("nan")), dict(regularisation=0.0), dict(regularisation=float("inf")),
               dict(attributes=torch.zeros((3, 2), device=DEV)), dict(attributes=torch.zeros(4, device=DEV)),
               dict(attributes=torch.zeros((4, 2))), dict(attributes=torch.zeros((4, 2), dtype=torch.int64, device=DEV)),
               dict(attributes=np.zeros((4, 2)))):
        with pytest.raises(ValueError):
            meshing.simplify_mesh(v, f, 0.5, **kw)
    nan = v.clone()
    nan[2, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        meshing.simplify_mesh(nan, f, 0.5)
    got = meshing.simplify_mesh(v, f, 0.6, origin=(-0.1, -0.1, -0.1), attributes=torch.zeros((4, 0), device=DEV))
    assert got.faces.shape == (2, 3) and got.attributes.shape == (4, 0)            # every vertex its own cluster
    e = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    for vv in (v, v[:0]):
        info = {}
        got = meshing.simplify_mesh(vv, e, 0.5, attributes=torch.ones((vv.shape[0], 2), device=DEV), _info=info)
        assert got.verts.shape == (0, 3) and got.verts.dtype == v.dtype and got.faces.shape == (0, 3)
        assert got.faces.dtype == got.vertex_cluster.dtype == got.face_src.dtype == torch.int64
        assert got.vertex_cluster.tolist() == [-1] * vv.shape[0] and got.face_src.shape == got.accepted.shape == (0,)
        assert got.accepted.dtype == torch.bool and got.attributes.shape == (0, 2) and info["clusters"] == 0
        got = meshing.simplify_to_faces(vv, e, 10)
        assert got.faces.shape == (0, 3) and got.attributes is None
