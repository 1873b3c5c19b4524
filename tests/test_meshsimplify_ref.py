"""CPU: the numpy restatement of the mesh simplification (tests/meshsimplify_ref.py) against the properties that make the
rule worth having: quadric placement keeps a crease where mean placement rounds it off, boundary quadrics keep the border
of an open surface where it otherwise shrinks, every output vertex lies in its cluster's cell, the output is a clean
mesh, and a second pass changes nothing.  Plus the guard of the GPU comparison: no accept decision of its inputs hangs on
the last bits.  The bounds are those of the float64 prototype of the rule; the figures it gave stand beside them."""
import numpy as np
import pytest

import meshsimplify_ref as S
import meshudf_ref as R


def _crease_clusters(v, f, r):
    """per output vertex: the share of its cluster's face weight (|n| / 2 per corner) on the half-plane that stays flat and
    on the rest (the half-plane that turns up, with the bent quads along the line) -> mask of the clusters where each side
    holds at least 15 %"""
    _, _, flat_normal, _ = S.fold_frame()
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = np.linalg.norm(n, axis=1)
    on_flat = np.abs(n @ flat_normal) / length >= 0.99
    weight = np.zeros((len(r.verts), 2))
    for k in range(3):
        np.add.at(weight, (r.vertex_cluster[f[:, k]], np.where(on_flat, 0, 1)), 0.5 * length)
    share = weight / weight.sum(1, keepdims=True)
    return (share >= 0.15).all(1)


def _crease_distance(points, cell):
    p, d, _, _ = S.fold_frame()
    return np.linalg.norm(np.cross(points - p, d), axis=1) / cell


def test_quadric_placement_keeps_a_crease_that_mean_placement_rounds_off():
    """prototype: 4608 -> 210 faces, 129 clusters, none at the mean; crease clusters 0.025 cell from the line with quadric
    placement, 0.22 - 0.30 cell with mean placement"""
    v, f = S.folded_sheet()
    cell = 0.17
    origin = S.lowered_origin(v, cell)
    q = S.simplify(v, f, cell, origin=origin)
    m = S.simplify(v, f, cell, origin=origin, placement="mean")
    assert (len(f), len(q.faces), q.clusters, int((~q.accepted).sum())) == (4608, 210, 129, 0)
    np.testing.assert_array_equal(q.faces, m.faces)
    np.testing.assert_array_equal(q.vertex_cluster, m.vertex_cluster)
    assert not m.accepted.any()
    crease = _crease_clusters(v, f, q)
    dq, dm = _crease_distance(q.verts[crease & q.accepted], cell), _crease_distance(m.verts[crease], cell)
    print(f"crease clusters {int(crease.sum())}: quadric max {dq.max():.4f} cell, mean min {dm.min():.4f} max {dm.max():.4f}")
    assert crease.any() and len(dq)                        # the two bounds below are about something
    assert dq.max() <= 0.05
    assert dm.min() >= 0.2


def test_few_clusters_fall_back_to_the_mean_on_a_finer_grid():
    """prototype: 5 of 280 clusters at cell 0.11"""
    v, f = S.folded_sheet()
    r = S.simplify(v, f, 0.11, origin=S.lowered_origin(v, 0.11))
    fallbacks = int((~r.accepted).sum())
    print(f"{fallbacks} of {r.clusters} clusters at the mean")
    assert len(r.verts) == r.clusters and fallbacks <= 0.05 * r.clusters


@pytest.mark.parametrize("boundary_weight", [1.0, 0.0])
def test_boundary_quadrics_keep_the_border_of_an_open_surface(boundary_weight):
    """flat axis-aligned sheet, cell 0.11.  prototype: with the boundary planes the box shrinks by 0.0026 cell per side and
    the area ratio is 0.9993; without them 0.31 cell and 0.918"""
    v, f = S.sheet()
    cell = 0.11
    r = S.simplify(v, f, cell, origin=S.lowered_origin(v, cell), boundary_weight=boundary_weight)
    shrink = np.concatenate([(r.verts.min(0) - v.min(0))[:2], (v.max(0) - r.verts.max(0))[:2]]) / cell
    ratio = R.area(r.verts, r.faces) / R.area(v, f)
    print(f"boundary_weight {boundary_weight}: shrink per side {shrink} cell, area ratio {ratio:.4f}")
    assert np.abs(r.verts[:, 2]).max() <= 1e-12
    if boundary_weight:
        assert shrink.max() <= 0.01 and ratio >= 0.995
    else:
        assert shrink.min() >= 0.25 and ratio <= 0.95


def _key_rows(points, case, grid):
    origin = S.bounding_origin(case["v"]) if case["origin"] is None else case["origin"]
    return S.keys_of(points, origin, case["cell"], grid), origin


@pytest.mark.parametrize("name", ["fold", "flat", "sphere"])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_structure(name, placement):
    case = S.cases()[name]
    v, f, cell = case["v"], case["f"], case["cell"]
    r = S.simplify(v, f, cell, origin=case["origin"], placement=placement, attributes=case["attributes"])
    assert len(r.faces) and len(r.faces) < len(f) and r.verts.dtype == v.dtype
    # every output vertex lies in its cluster's cell, hence within the cell's diagonal of each of its input vertices
    key_out, origin = _key_rows(r.verts, case, r.grid)
    key_in, _ = _key_rows(v, case, r.grid)
    used = r.vertex_cluster >= 0
    assert (key_out >= 0).all() and (key_in >= 0).all()
    np.testing.assert_array_equal(key_out[r.vertex_cluster[used]], key_in[used])
    assert np.linalg.norm(v[used] - r.verts[r.vertex_cluster[used]], axis=1).max() <= np.sqrt(3.0) * cell
    # a clean mesh
    t = r.faces
    assert ((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])).all()
    assert len(np.unique(np.sort(t, 1), axis=0)) == len(t)
    np.testing.assert_array_equal(np.unique(t), np.arange(len(r.verts)))
    assert (np.diff(r.face_src) > 0).all() and r.face_src.min() >= 0 and r.face_src.max() < len(f)
    np.testing.assert_array_equal(r.faces, r.vertex_cluster[f[r.face_src]])
    assert r.attributes.shape == (len(r.verts), 3) and r.accepted.shape == (len(r.verts),)
    assert (r.attributes >= case["attributes"].min()).all() and (r.attributes <= case["attributes"].max()).all()
    # a second pass over the output with the same grid changes neither count
    again = S.simplify(r.verts, r.faces, cell, origin=origin, placement=placement)
    assert (len(again.verts), len(again.faces)) == (len(r.verts), len(r.faces))


def test_default_origin_puts_a_flat_part_at_the_minimum_on_a_cell_wall():
    """why the sheets above get an origin a fraction of a cell below the minimum: with the default origin the flat half of
    the folded sheet lies in the wall z = origin, and the accept test of its clusters hangs on the last bit"""
    v, f = S.folded_sheet()
    r = S.simplify(v, f, 0.17)
    assert r.wall_margin < 1e-9
    assert len(r.faces) > 0 and (S.keys_of(r.verts, S.bounding_origin(v), 0.17, r.grid) >= 0).all()


@pytest.mark.parametrize("name", list(S.cases()))
def test_gpu_inputs_keep_accept_decisions_away_from_the_walls(name):
    """the GPU comparison asks for equal accept decisions and positions to 1e-9 cell: no quadric solution of its inputs may
    lie within 1e-6 cell of a wall of its cell"""
    case = S.cases()[name]
    r = S.simplify(case["v"], case["f"], case["cell"], origin=case["origin"])
    print(f"{name}: {len(case['f'])} -> {len(r.faces)} faces, {r.clusters} clusters, margin {r.wall_margin:.3g} cell")
    assert r.wall_margin > 1e-6


def test_key_arithmetic_patch_is_exact_near_2_to_the_59():
    v, f, cell, origin = S.key_patch()
    grid = S.grid_dims(v, origin, cell)
    assert (grid == S.MAX_GRID - 1).all()
    key = S.keys_of(v, origin, cell, grid)
    assert key.min() > 2 ** 59 and key.max() < 2 ** 60
    r = S.simplify(v, f, cell, origin=origin)
    assert 0 < len(r.faces) < len(f) == 200 and r.wall_margin > 1e-6


def test_simplify_to_faces_meets_its_target():
    v, f = S.sphere_mesh()
    for target in (1000, 200, 20):
        n, cell = S.bisect_cells(v, f, target)
        r = S.simplify_to_faces(v, f, target)
        print(f"target {target}: {n} cells, {len(r.faces)} faces")
        assert n >= 2 and 0 < len(r.faces) <= target and len(r.faces) == S.count_faces(v, f, cell)
    assert S.simplify_to_faces(v, f, len(f)) is None


def test_argument_errors_and_empty_meshes():
    v, f = S.sheet(4)
    with pytest.raises(ValueError):
        S.simplify(v, f, 0.1, origin=v.min(0) + 0.01)
    with pytest.raises(ValueError):
        S.simplify(v, f, 1e-7)                                     # more than 2^20 cells along an axis
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        S.simplify(bad, f, 0.1)
    r = S.simplify(v, f[:0], 0.1)
    assert len(r.verts) == 0 and len(r.faces) == 0 and (r.vertex_cluster == -1).all()
    r = S.simplify(v, f, 100.0)                                    # one cluster: every face collapses
    assert len(r.verts) == 0 and len(r.faces) == 0 and r.clusters == 1 and (r.vertex_cluster == -1).all()
