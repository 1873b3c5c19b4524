"""GPU: intersecting faces (neuraludf_amd/evaluation.py MeshIndex.intersections / self_intersections / mesh_intersections,
csrc/meshintersect.hip) against the plain-Python restatement (tests/meshintersect_ref.py) bit for bit in the pair set and
the kinds, in self mode and against a second mesh; independence of the cell size, of the run and of the face order; the
two clean-up steps built on it (meshclean.drop_self_intersections, close_holes_checked), extract_udf_mesh's switches and
the two CLI words; and one size beyond the restatement's reach, held against cast_rays.  The restatement of an input is
computed once."""
import functools

import numpy as np
import pytest
import torch

import meshhole_cases
import meshhole_ref
import meshintersect_cases as cases
import meshintersect_ref as R
import meshray_ref
from common import build_modules

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _input(name):
    """(verts, faces, the restatement's pairs) of a named input; read only"""
    if name == "random":
        verts, faces = R.random_triangles(300, 0.2, 0)
    elif name == "spheres":
        verts, faces = R.merged(*R.two_spheres(2, 0.3))
    elif name == "sphere":
        verts, faces = (np.asarray(x) for x in meshray_ref.icosphere(2))
    elif name == "sheet":
        verts, faces = cases.spiked_sheet()[:2]
    else:
        verts, faces = cases.HAND[name][:2]
    return verts, faces, R.pairs(verts, faces)


def _as_list(res):
    return [(a, b, k) for (a, b), k in zip(res.pairs.cpu().tolist(), res.kind.cpu().tolist())]


INPUTS = ["random", "spheres", "sphere", "sheet"] + sorted(cases.HAND)


@pytest.mark.parametrize("name", INPUTS)
def test_self_mode_equals_the_restatement(name):
    from neuraludf_amd import evaluation as E
    verts, faces, want = _input(name)
    res = E.self_intersections(_dev(verts), _dev(faces))
    assert res.pairs.dtype == torch.int64 and res.kind.dtype == torch.int8 and res.face_mask.dtype == torch.bool
    assert res.pairs.shape == (len(want), 2) and res.face_mask.shape == (len(faces),)
    assert _as_list(res) == want
    mask = np.zeros(len(faces), bool)
    mask[[x for a, b, _ in want for x in (a, b)]] = True
    assert np.array_equal(res.face_mask.cpu().numpy(), mask)
    if name in cases.HAND:
        assert want == cases.HAND[name][2]
    if name == "spheres":
        assert len(want) > 50
    if name == "sphere":
        assert want == []


def test_two_meshes_equal_the_restatement_and_the_merged_self_run():
    from neuraludf_amd import evaluation as E
    a, b = R.two_spheres(2, 0.3)
    fa = len(a[1])
    want = R.pairs(a[0], a[1], other=b)
    assert want == [(x, y - fa, k) for x, y, k in _input("spheres")[2]]        # a sphere does not cross itself
    res = E.mesh_intersections((_dev(a[0]), _dev(a[1])), (_dev(b[0]), _dev(b[1])))
    assert _as_list(res) == want
    for mask, col in ((res.mask_a, 0), (res.mask_b, 1)):
        assert sorted(set(p[col] for p in want)) == torch.nonzero(mask).reshape(-1).tolist()
    # through an index of either mesh: the index holds the second faces of the pairs, the queries the first
    ib = E.MeshIndex(_dev(b[0]), _dev(b[1]))
    assert _as_list(ib.intersections((_dev(a[0]), _dev(a[1])))) == want
    assert _as_list(E.mesh_intersections((_dev(a[0]), _dev(a[1])), ib)) == want
    # an index stays usable for the other queries afterwards
    assert ib.cast(_dev(np.zeros((1, 3))), _dev(np.array([[0.0, 0.0, 1.0]])), mode="count").tolist() == [1]
    # random triangles against the sphere, more queries than faces and the other way round
    rv, rf = R.random_triangles(300, 0.4, 3)
    rv = rv * 2.4 - 1.2
    want = R.pairs(rv, rf, other=a)
    assert len(want) > 20
    got = E.mesh_intersections((_dev(rv), _dev(rf)), (_dev(a[0]), _dev(a[1])))        # indexes a: 320 faces > 300
    assert _as_list(got) == want
    back = E.mesh_intersections((_dev(a[0]), _dev(a[1])), (_dev(rv), _dev(rf)))        # indexes a again, pairs turned round
    assert sorted((b_, a_) for a_, b_ in back.pairs.cpu().tolist()) == [(x, y) for x, y, _ in want]
    assert back.pairs.cpu().tolist() == sorted(back.pairs.cpu().tolist())
    assert sorted(back.kind.cpu().tolist()) == sorted(k for *_, k in want)


@pytest.mark.parametrize("name", ["random", "spheres", "sheet"])
def test_same_bytes_for_every_cell_and_run(name):
    from neuraludf_amd import evaluation as E
    verts, faces, want = _input(name)
    base = E.MeshIndex(_dev(verts), _dev(faces))
    assert abs(base.cell / R.default_cell(verts, faces) - 1.0) < 1e-12          # torch's mean against numpy's
    first = base.intersections()
    for factor in (0.5, 1.0, 4.0):
        res = E.MeshIndex(_dev(verts), _dev(faces), cell=factor * base.cell).intersections()
        for x, y in zip(res, first):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), factor
    again = base.intersections()
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(again, first))
    assert _as_list(first) == want


def test_face_relabelling_permutes_the_result():
    from neuraludf_amd import evaluation as E
    verts, faces, want = _input("spheres")
    perm = np.random.default_rng(11).permutation(len(faces))          # new face i is old face perm[i]
    res = E.self_intersections(_dev(verts), _dev(faces[perm]))
    got = sorted((min(perm[a], perm[b]), max(perm[a], perm[b]), k) for a, b, k in _as_list(res))
    assert got == want
    assert np.array_equal(res.face_mask.cpu().numpy()[np.argsort(perm)],
                          E.self_intersections(_dev(verts), _dev(faces)).face_mask.cpu().numpy())


def test_refusals_by_message():
    from neuraludf_amd import evaluation as E
    verts, faces, want = _input("spheres")
    index = E.MeshIndex(_dev(verts), _dev(faces))
    with pytest.raises(ValueError, match=f"{len(want)} intersecting pairs exceed max_pairs={len(want) - 1}"):
        index.intersections(max_pairs=len(want) - 1)
    assert _as_list(index.intersections(max_pairs=len(want))) == want            # the refusal left the index usable
    with pytest.raises(ValueError, match="max_pairs"):
        index.intersections(max_pairs=-1)
    with pytest.raises(ValueError, match="other"):
        index.intersections(other=5)
    with pytest.raises(ValueError, match="out of range"):
        index.intersections(other=(_dev(verts), _dev(faces + len(verts))))
    with pytest.raises(ValueError, match="not both"):
        E.self_intersections(_dev(verts), _dev(faces), index=index)
    with pytest.raises(ValueError, match="needs"):
        E.self_intersections()
    empty = index.intersections(other=(_dev(verts), _dev(faces[:0])))
    assert empty.pairs.shape == (0, 2) and empty.kind.shape == (0,) and not bool(empty.face_mask.any())


def test_drop_self_intersections():
    from neuraludf_amd import evaluation as E, meshclean, meshing
    assert meshing.drop_self_intersections is meshclean.drop_self_intersections
    verts, faces, want = _input("spheres")
    v, f, n = meshclean.drop_self_intersections(_dev(verts), _dev(faces))
    hit = sorted(set(x for a, b, _ in want for x in (a, b)))
    assert n == len(hit) and f.shape[0] == len(faces) - n
    keep = np.ones(len(faces), bool)
    keep[hit] = False
    assert np.array_equal(v.cpu().numpy()[f.cpu().numpy()], verts[faces[keep]])      # the same triangles, in order
    assert E.self_intersections(v, f).pairs.shape[0] == 0
    assert meshclean.drop_self_intersections(v, f)[2] == 0
    # by kind: the flat fold is coplanar, the corner in a face uncertain
    for name, kinds, dropped in (("flat_fold", ("crossing",), 0), ("flat_fold", ("crossing", "coplanar"), 2),
                                 ("corner_in_face", ("crossing", "coplanar"), 0), ("corner_in_face", "uncertain", 2)):
        cv, cf, _ = _input(name)
        assert meshclean.drop_self_intersections(_dev(cv), _dev(cf), kinds)[2] == dropped, (name, kinds)
    with pytest.raises(ValueError, match="kinds"):
        meshclean.drop_self_intersections(_dev(verts), _dev(faces), ("touching",))


def _border_and_multi(faces, n_verts):
    a, b = faces.reshape(-1), np.roll(faces, -1, 1).reshape(-1)
    key, counts = np.unique(np.minimum(a, b) * n_verts + np.maximum(a, b), return_counts=True)
    return set(key[counts == 1].tolist()), set(key[counts > 2].tolist())


def test_close_holes_checked_takes_the_spiked_patch_back():
    from neuraludf_amd import meshclean, meshing
    assert meshing.close_holes_checked is meshclean.close_holes_checked
    verts, faces, spiked_rim, clear_rim = cases.spiked_sheet()
    V, F = len(verts), len(faces)
    plain = meshclean.close_holes(_dev(verts), _dev(faces), 32)
    loops = meshclean.border_loops(_dev(verts), _dev(faces))
    off, lv = loops.loop_off.cpu().numpy(), loops.loop_vertex.cpu().numpy()
    loop_of = lambda vertex: [l for l in range(len(off) - 1) if vertex in lv[off[l]:off[l + 1]]]
    (spiked,), (clear,) = loop_of(spiked_rim), loop_of(clear_rim)
    status = plain.status.cpu().numpy()
    assert status[spiked] == meshhole_ref.FILLED and status[clear] == meshhole_ref.FILLED
    # what the restatements say of the closed mesh: the spike crosses faces of the spiked hole's patch, and of no other
    closed_ref = meshhole_ref.close_holes(verts, faces, max_edges=32)
    np.testing.assert_array_equal(plain.faces.cpu().numpy(), closed_ref.faces)
    want = [p for p in R.pairs(verts, closed_ref.faces) if p[2] in (R.CROSSING, R.COPLANAR)]
    new_loop = plain.new_face_loop.cpu().numpy()
    want_back = sorted(set(int(new_loop[x - F]) for a, b, _ in want for x in (a, b) if x >= F))
    assert spiked in want_back and clear not in want_back
    assert any(k == R.CROSSING and b >= F and new_loop[b - F] == spiked and a >= F - 2 for a, b, k in want)

    out, back = meshclean.close_holes_checked(_dev(verts), _dev(faces), 32)
    assert back.tolist() == want_back and back.dtype == torch.int64
    got, got_loop = out.faces.cpu().numpy(), out.new_face_loop.cpu().numpy()
    keep = ~np.isin(new_loop, want_back)
    np.testing.assert_array_equal(got, np.concatenate([faces, closed_ref.faces[F:][keep]]))
    np.testing.assert_array_equal(got_loop, new_loop[keep])
    np.testing.assert_array_equal(out.status.cpu().numpy(), status)
    assert clear in got_loop and spiked not in got_loop
    # the kept result has the properties of a closed hole: the kept loops lost their border, the others kept theirs, no
    # edge gained a third face, one more Euler unit per kept patch, the old faces first, loop by loop
    e = meshclean.mesh_edges(_dev(faces), V).edges.cpu().numpy()
    key, ledge = e[:, 0] * V + e[:, 1], loops.loop_edge.cpu().numpy()
    border0, multi0 = _border_and_multi(faces, V)
    border1, multi1 = _border_and_multi(got, V)
    kept = [l for l in range(len(status)) if status[l] == meshhole_ref.FILLED and l not in want_back]
    for l in range(len(status)):
        keys = set(key[ledge[off[l]:off[l + 1]]].tolist())
        assert keys <= border0
        assert (not keys & border1) if l in kept else keys <= border1, l
    assert multi1 <= multi0
    assert meshhole_cases.euler(got) == meshhole_cases.euler(faces) + len(kept)
    assert len(got) == F + sum(int(off[l + 1] - off[l] - 2) for l in kept)
    assert np.all(np.diff(got_loop) >= 0)
    # nothing of the dropped kinds is left between a kept patch and the rest
    from neuraludf_amd import evaluation as E
    left = E.self_intersections(_dev(verts), out.faces)
    assert not bool(((left.kind != R.UNCERTAIN) & (left.pairs >= F).any(1)).any())
    # a sheet without the spike keeps both patches
    plain_v, plain_f = verts[:-4], faces[:-2]
    out2, back2 = meshclean.close_holes_checked(_dev(plain_v), _dev(plain_f), 32)
    assert back2.numel() == 0
    np.testing.assert_array_equal(out2.faces.cpu().numpy(), meshclean.close_holes(_dev(plain_v), _dev(plain_f), 32).faces.cpu().numpy())


def test_extract_udf_mesh_switches():
    from neuraludf_amd import meshclean, meshing
    from neuraludf_amd.models import fields
    udf = build_modules(fields, seed=0)["udf"].to(DEV)
    v0, f0 = meshing.extract_udf_mesh(udf, 33, close_holes=32)
    # both switches off: the steps as they were, through functions this change does not touch
    raw_v, raw_f = meshing.extract_udf_mesh(udf, 33)
    assert v0.tobytes() == raw_v.tobytes()
    assert f0.tobytes() == meshclean.close_holes(_dev(raw_v), _dev(raw_f), 32).faces.cpu().numpy().tobytes()
    v1, f1 = meshing.extract_udf_mesh(udf, 33, close_holes=32, close_holes_check=False, drop_self_intersections=False)
    assert v1.tobytes() == v0.tobytes() and f1.tobytes() == f0.tobytes()
    v2, f2 = meshing.extract_udf_mesh(udf, 33, close_holes=32, close_holes_check=True)
    want2 = meshclean.close_holes_checked(_dev(raw_v), _dev(raw_f), 32)[0].faces
    assert v2.tobytes() == raw_v.tobytes() and f2.tobytes() == want2.cpu().numpy().tobytes()
    v3, f3 = meshing.extract_udf_mesh(udf, 33, drop_self_intersections=True)
    wv, wf, n = meshclean.drop_self_intersections(_dev(raw_v), _dev(raw_f))
    print(f"N=33: {len(raw_f)} faces, {n} dropped, {len(f0) - len(f2)} patch faces taken back")
    assert v3.tobytes() == wv.cpu().numpy().tobytes() and f3.tobytes() == wf.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="close_holes_check needs close_holes"):
        meshing.extract_udf_mesh(udf, 33, close_holes_check=True)


def test_cli_words(tmp_path, capsys):
    from neuraludf_amd import evaluation as E, meshing
    a, b = R.two_spheres(2, 0.3)
    verts, faces, want = _input("spheres")
    v32 = verts.astype(np.float32)                                # a PLY file stores float32
    want32 = R.pairs(v32.astype(np.float64), faces)
    meshing.write_ply(tmp_path / "m.ply", v32, faces)
    assert E.main(["intersections", "--mesh", str(tmp_path / "m.ply"), "--out", str(tmp_path / "flag.ply")]) == 0
    text = capsys.readouterr().out
    n = {k: sum(1 for p in want32 if p[2] == c) for k, c in (("crossing", 1), ("coplanar", 2), ("uncertain", 3))}
    flagged = len(set(x for p in want32 for x in p[:2]))
    assert (f"pairs: {len(want32)}; crossing: {n['crossing']}; coplanar: {n['coplanar']}; uncertain: {n['uncertain']}; "
            f"flagged faces: {flagged} of {len(faces)}.") in text
    fv, ff, colors = meshing.read_ply(tmp_path / "flag.ply", with_colors=True)
    assert np.array_equal(ff, faces) and colors.shape == (len(verts), 3)
    red = (colors == np.array([255, 0, 0])).all(1)
    hit = np.zeros(len(verts), bool)
    hit[faces[sorted(set(x for p in want32 for x in p[:2]))].reshape(-1)] = True
    assert np.array_equal(red, hit)
    meshing.write_ply(tmp_path / "a.ply", a[0].astype(np.float32), a[1])
    meshing.write_ply(tmp_path / "b.ply", b[0].astype(np.float32), b[1])
    assert E.main(["intersections", "--mesh", str(tmp_path / "a.ply"), "--other", str(tmp_path / "b.ply")]) == 0
    two = R.pairs(a[0].astype(np.float32).astype(np.float64), a[1], other=(b[0].astype(np.float32).astype(np.float64), b[1]))
    assert f"pairs: {len(two)}; crossing: {sum(1 for p in two if p[2] == 1)};" in capsys.readouterr().out
    # the mesh tool: both switches
    sv, sf, _, _ = cases.spiked_sheet()
    meshing.write_ply(tmp_path / "sheet.ply", sv.astype(np.float32), sf)
    assert meshing.main([str(tmp_path / "sheet.ply"), str(tmp_path / "closed.ply"), "--close-holes", "32",
                         "--close-holes-check"]) == 0
    text = capsys.readouterr().out
    assert "close_holes_check: " in text and "patches taken back (loops [" in text and "close_holes: " in text
    assert len(meshing.read_ply(tmp_path / "closed.ply")[1]) >= len(sf) + 4
    assert meshing.main([str(tmp_path / "m.ply"), str(tmp_path / "dropped.ply"), "--drop-self-intersections"]) == 0
    assert f"drop_self_intersections: {flagged} faces dropped" in capsys.readouterr().out
    dv, df = meshing.read_ply(tmp_path / "dropped.ply")
    assert len(df) == len(faces) - flagged
    assert E.self_intersections(_dev(dv), _dev(df)).pairs.shape[0] == 0
    with pytest.raises(SystemExit):
        meshing.main([str(tmp_path / "m.ply"), str(tmp_path / "x.ply"), "--close-holes-check"])


def test_large_sphere_against_its_shifted_copy_confirmed_by_rays():
    """20 480 faces twice, beyond the restatement's reach: two runs give equal bytes, no sphere crosses itself, and every
    CROSSING pair is confirmed by cast_rays: an edge of one face, cast as a ray over t in [0, 1] from either end against
    the crossed faces of the other sphere, hits the other face of the pair first"""
    from neuraludf_amd import evaluation as E
    v, f = (np.asarray(x) for x in meshray_ref.icosphere(5))
    F = len(f)
    assert F == 20480
    vb = v + 0.5 * np.array(R.SHIFT_DIRECTION)
    verts, faces = R.merged((v, f), (vb, f))
    index = E.MeshIndex(_dev(verts), _dev(faces))
    res, again = index.intersections(), index.intersections()
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(res, again))
    pairs, kind = res.pairs.cpu().numpy(), res.kind.cpu().numpy()
    assert len(pairs) > 500 and np.all(pairs[:, 0] < F) and np.all(pairs[:, 1] >= F)
    assert np.all(pairs[:-1, 0] * 2 * F + pairs[:-1, 1] < pairs[1:, 0] * 2 * F + pairs[1:, 1])        # sorted, each once
    assert (kind == R.CROSSING).mean() > 0.99
    two = E.mesh_intersections((_dev(v), _dev(f)), (_dev(vb), _dev(f)))
    assert np.array_equal(two.pairs.cpu().numpy(), pairs - np.array([0, F])) and np.array_equal(two.kind.cpu().numpy(), kind)
    cross = pairs[kind == R.CROSSING]
    confirmed = np.zeros(len(cross), bool)
    for src, dst in ((0, 1), (1, 0)):                        # edges of the pair's face `src` against its face `dst`
        targets, inverse = np.unique(cross[:, dst], return_inverse=True)
        sub = E.MeshIndex(_dev(verts), _dev(faces[targets]))
        tri = verts[faces[cross[:, src]]]                     # [P, 3, 3]
        for k in range(3):
            p, q = tri[:, k], tri[:, (k + 1) % 3]
            for o, d in ((p, q - p), (q, p - q)):
                hit = sub.cast(_dev(o), _dev(d), t_min=0.0, t_max=1.0).face.cpu().numpy()
                confirmed |= hit == inverse
    assert confirmed.all(), (int((~confirmed).sum()), len(cross))
