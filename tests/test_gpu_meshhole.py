"""GPU: the hole closing (neuraludf_amd/meshclean.py border_loops / close_holes, csrc/meshhole.hip) against the numpy
restatement (tests/meshhole_ref.py) bit for bit: every entry point through the descriptor -- link, each rank round, count,
triangulate -- on the hand-built meshes of tests/meshhole_cases.py, then close_holes end to end with the properties a
closed hole must have, the network through extract_udf_mesh, and the CLI.  The restatement of a case is computed once."""
import functools
import math

import numpy as np
import pytest
import torch

import meshhole_cases as cases
import meshhole_ref as ref
from common import build_modules

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

CASES = {
    "disc3": lambda: cases.annulus(3), "disc4": lambda: cases.annulus(4), "disc5": lambda: cases.annulus(5),
    "disc7": lambda: cases.annulus(7), "bow_tie": cases.bow_tie, "pinched": cases.pinched_holes, "fin": cases.fin,
    "repeated_vertex": cases.repeated_vertex_face, "strip": cases.strip_over_hole, "shared_diagonal": cases.shared_diagonal,
    "half_flipped": lambda: (cases.sphere_patch((3, 5, 6, 17))[0], cases.flip_half(cases.sphere_patch((3, 5, 6, 17))[1])),
    "sphere": cases.sphere_patch, "saddle12": lambda: cases.annulus(12, saddle=0.8),
}


@functools.lru_cache(maxsize=None)
def _case(name, max_edges=64):
    """(verts, faces, the restatement's stages) of a case; read only"""
    verts, faces = CASES[name]()
    tb = ref.table(faces, len(verts))
    lnk = ref.link(faces, tb)
    tabs = [ref.rank_init(lnk)]
    for r in range(ref.rank_rounds(len(lnk) // 2)):
        tabs.append(ref.rank_round(tabs[-1], r))
    lp = ref.loops(tb, lnk)
    per, status, cnt = ref.count(verts, tb, lp, max_edges)
    new, status2 = ref.triangulate(verts, faces, tb, lp, status, cnt)
    return verts, faces, dict(tb=tb, link=lnk, tabs=tabs, loops=lp, perimeter=per, status=status, count=cnt, new=new,
                              status2=status2)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges(faces, n_verts):
    """(border edges, edges with more than two faces) of a face array as sets of keys"""
    a, b = faces.reshape(-1), np.roll(faces, -1, 1).reshape(-1)
    key, counts = np.unique(np.minimum(a, b) * n_verts + np.maximum(a, b), return_counts=True)
    return set(key[counts == 1].tolist()), set(key[counts > 2].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_each_entry_point_through_the_descriptor(name):
    from neuraludf_amd import meshclean
    from neuraludf_amd._lib import call, ptr
    verts, faces, want = _case(name)
    tb, lp = want["tb"], want["loops"]
    v, f = _dev(verts), _dev(faces)
    table = meshclean._mesh_edges(f, len(verts))
    np.testing.assert_array_equal(table.edges[:, :4].cpu().numpy(), np.stack([tb.u, tb.v, tb.count, tb.face0], 1))
    d = meshclean._topo(f, len(verts), table)
    rounds = []
    loops = meshclean._hole_loops(d, table, len(verts), _rounds=rounds)
    # link and every rank round
    np.testing.assert_array_equal(loops[5][2].cpu().numpy(), want["link"])
    assert len(rounds) == len(want["tabs"]) - 1 == ref.rank_rounds(len(tb.bedge))
    for r, (got, exp) in enumerate(zip(rounds, want["tabs"][1:])):
        np.testing.assert_array_equal(got.cpu().numpy(), exp, err_msg=f"rank round {r}")
    # the glue: the loops of the walk
    for got, exp in zip(loops[:5], (lp.loop_off, lp.loop_vertex, lp.loop_edge, lp.closed.astype(np.uint8), lp.edge_loop)):
        np.testing.assert_array_equal(got.cpu().numpy(), exp)
    # count
    pos = v.double().contiguous()
    per, status, cnt = meshclean._hole_count(d, pos, loops, 64, None)
    assert per.cpu().numpy().tobytes() == want["perimeter"].tobytes()
    np.testing.assert_array_equal(status.cpu().numpy(), want["status"])
    np.testing.assert_array_equal(cnt.cpu().numpy(), want["count"])
    # triangulate
    n_new = int(cnt.sum())
    if n_new:
        off = torch.cumsum(cnt, 0) - cnt
        new = torch.full((n_new, 3), -7, dtype=torch.int64, device=DEV)
        d.new_off, d.new_faces, d.n_new = ptr(off), ptr(new), n_new
        call("nudf_meshhole_triangulate", d)
        np.testing.assert_array_equal(new.cpu().numpy(), want["new"])              # every row written: none is -7
        np.testing.assert_array_equal(status.cpu().numpy(), want["status2"])
    if name == "sphere":
        n = np.diff(lp.loop_off)
        assert sorted(n[want["status2"] == ref.FILLED].tolist()) == [3, 4, 5, 6, 7, 17, 63, 64]
        assert sorted(n[want["status2"] == ref.TOO_MANY_EDGES].tolist()) == [65, 176]
    if name == "saddle12":                                   # the minimum-area triangulation of a saddle is no fan
        inner = want["new"][np.all(want["new"] < 12, 1)]
        assert len(inner) == 10 and np.bincount(inner.reshape(-1), minlength=12).max() < 10


def _close(name, **kw):
    from neuraludf_amd import meshclean
    verts, faces, _ = _case(name)
    info = {}
    out = meshclean.close_holes(_dev(verts), _dev(faces), _info=info, **kw)
    want = ref.close_holes(verts, faces, **kw)
    got_faces = out.faces.cpu().numpy()
    np.testing.assert_array_equal(got_faces, want.faces)
    np.testing.assert_array_equal(out.new_face_loop.cpu().numpy(), want.new_face_loop)
    np.testing.assert_array_equal(out.status.cpu().numpy(), want.status)
    assert out.status.dtype == torch.int8 and out.faces.dtype == torch.int64
    return verts, faces, out, info["loops"], got_faces


def _check_properties(verts, faces, out, loops, got):
    """what a closed hole must look like, whatever the restatement says"""
    V = len(verts)
    status = out.status.cpu().numpy()
    off, ledge = loops.loop_off.cpu().numpy(), loops.loop_edge.cpu().numpy()
    from neuraludf_amd import meshclean
    e = meshclean.mesh_edges(_dev(faces), V).edges.cpu().numpy()
    key = e[:, 0] * V + e[:, 1]
    border0, multi0 = _edges(faces, V)
    border1, multi1 = _edges(got, V)
    for l in range(len(status)):
        keys = set(key[ledge[off[l]:off[l + 1]]].tolist())
        assert keys <= border0
        if status[l] == ref.FILLED:
            assert not keys & border1, l                      # a filled loop leaves no border edge of its own
        else:
            assert keys <= border1, l                         # every other loop keeps all of its
    assert multi1 <= multi0                                   # no edge gains a third face
    filled = int((status == ref.FILLED).sum())
    assert cases.euler(got) == cases.euler(faces) + filled
    assert len(got) == len(faces) + int(((off[1:] - off[:-1] - 2)[status == ref.FILLED]).sum())
    assert np.array_equal(got[:len(faces)], faces)
    assert np.all(np.diff(out.new_face_loop.cpu().numpy()) >= 0)   # loop by loop in loop-id order


@pytest.mark.parametrize("name", list(CASES))
def test_close_holes_end_to_end(name):
    verts, faces, out, loops, got = _close(name, max_edges=64)
    _check_properties(verts, faces, out, loops, got)
    n = (loops.loop_off[1:] - loops.loop_off[:-1]).cpu().numpy()
    status = out.status.cpu().numpy()
    if name == "sphere":
        assert sorted(n[status == ref.TOO_MANY_EDGES].tolist()) == [65, 176] and (status == ref.FILLED).sum() == 8
    if name == "fin":
        assert np.all(status == ref.OPEN_CHAIN) and not loops.closed.any() and len(got) == len(faces)
    if name == "repeated_vertex":
        assert sorted(n[status == ref.OPEN_CHAIN].tolist()) == [1, 3]
    if name == "pinched":
        assert n[status == ref.REPEATED_VERTEX].tolist() == [8]
    if name == "bow_tie":
        assert sorted(n[status == ref.FILLED].tolist()) == [4, 4, 5, 5]
    if name == "shared_diagonal":                             # the second patch would share the first one's diagonal
        assert sorted(status.tolist()) == [ref.FILLED] * 3 + [ref.DUPLICATE] and _edges(got, len(verts))[1] == set()
    if name == "strip":                                     # a diagonal that is an edge already, a triangle that is a face
        assert sorted(n[(status == ref.DUPLICATE) & (n <= 4)].tolist()) == [3, 3, 4]


def test_border_loops_public_surface():
    from neuraludf_amd import meshclean, meshing
    assert meshing.border_loops is meshclean.border_loops and meshing.close_holes is meshclean.close_holes
    verts, faces, want = _case("sphere")
    got = meshing.border_loops(_dev(verts).float(), _dev(faces))
    lp = want["loops"]
    ref32 = ref.count(verts.astype(np.float32).astype(np.float64), want["tb"], lp, 64)[0]
    for a, b in zip(got, (lp.loop_off, lp.loop_vertex, lp.loop_edge, lp.closed, ref32, lp.edge_loop)):
        assert a.cpu().numpy().tobytes() == np.ascontiguousarray(b).tobytes()
    assert got.closed.dtype == torch.bool and got.perimeter.dtype == torch.float64
    closed = meshing.border_loops(*map(_dev, (np.array([[0., 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]),
                                             np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]]))))
    assert closed.closed.numel() == 0 and closed.loop_off.tolist() == [0] and closed.edge_loop.tolist() == [-1] * 6


def test_max_edges_and_max_perimeter():
    from neuraludf_amd import meshclean
    verts, faces, out, loops, got = _close("sphere", max_edges=7)
    n = (loops.loop_off[1:] - loops.loop_off[:-1]).cpu().numpy()
    assert np.array_equal(out.status.cpu().numpy() == ref.FILLED, n <= 7)
    _check_properties(verts, faces, out, loops, got)
    per = loops.perimeter.cpu().numpy()
    a, b = np.argsort(per)[:2]
    assert per[a] < per[b]
    verts, faces, out, loops, got = _close("sphere", max_edges=64, max_perimeter=0.5 * (per[a] + per[b]))
    status = out.status.cpu().numpy()
    assert status[a] == ref.FILLED and status[b] == ref.PERIMETER and (status == ref.FILLED).sum() == 1
    _check_properties(verts, faces, out, loops, got)
    v, f = _dev(verts), _dev(faces)
    for bad in (2, 65, 0, 3.5, "4", None):
        with pytest.raises(ValueError, match="max_edges"):
            meshclean.close_holes(v, f, max_edges=bad)
    assert meshclean.MAX_HOLE_EDGES == 64
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_perimeter"):
            meshclean.close_holes(v, f, max_perimeter=bad)
    with pytest.raises(ValueError, match="max_loop"):
        meshclean.fill_holes(v, f, max_loop=5)                # fill_holes keeps its own bound
    empty = meshclean.close_holes(v, f[:0])
    assert empty.faces.shape == (0, 3) and empty.status.numel() == 0 and empty.new_face_loop.numel() == 0


def test_three_loops_close_the_sphere_patch_like_fill_holes():
    from neuraludf_amd import meshclean
    verts, faces = cases.sphere_patch((3,) * 8)
    # close the outer border first so that only the 3-loops are border: a fan to an apex
    tb = ref.table(faces, len(verts))
    lp = ref.loops(tb, ref.link(faces, tb))
    outer = int(np.argmax(np.diff(lp.loop_off)))
    ring = lp.loop_vertex[lp.loop_off[outer]:lp.loop_off[outer + 1]]
    verts = np.concatenate([verts, [[0.0, 0.0, -2.0]]])
    faces = np.concatenate([faces, np.stack([ring, np.roll(ring, -1), np.full(len(ring), len(verts) - 1)], 1)])
    v, f = _dev(verts), _dev(faces)
    out = meshclean.close_holes(v, f, max_edges=3)
    filled, n_filled = meshclean.fill_holes(v, f, max_loop=3)
    status = out.status.cpu().numpy()
    assert len(status) == 8 and np.all(status == ref.FILLED) and n_filled == 8
    assert _edges(out.faces.cpu().numpy(), len(verts)) == (set(), set())               # closed
    assert _edges(filled.cpu().numpy(), len(verts)) == (set(), set())
    np.testing.assert_array_equal(out.faces.cpu().numpy(), ref.close_holes(verts, faces, max_edges=3).faces)


def _consistent(faces):
    """every edge with two faces is run through once in each direction"""
    a, b = faces.reshape(-1), np.roll(faces, -1, 1).reshape(-1)
    n = int(faces.max()) + 1
    und, inv, cnt = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_inverse=True, return_counts=True)
    forward = np.bincount(inv, weights=(a < b).astype(np.float64), minlength=len(und))
    return bool(np.all(forward[cnt == 2] == 1))


def test_winding_follows_the_neighbours():
    from neuraludf_amd import meshclean
    verts, faces, _ = _case("sphere")
    v = _dev(verts)
    oriented = meshclean.orient_faces(v, _dev(faces)).faces
    assert _consistent(oriented.cpu().numpy())
    out = meshclean.close_holes(v, oriented, max_edges=64)
    assert (out.status == ref.FILLED).sum() == 8 and _consistent(out.faces.cpu().numpy())
    # the other winding of the whole mesh: the patches turn with it
    out2 = meshclean.close_holes(v, oriented[:, [0, 2, 1]].contiguous(), max_edges=64)
    assert _consistent(out2.faces.cpu().numpy())
    np.testing.assert_array_equal(out2.faces[len(faces):].cpu().numpy(), out.faces[len(faces):][:, [0, 2, 1]].cpu().numpy())
    # half the faces flipped: the vote follows the majority, as the restatement states it
    flipped = cases.flip_half(oriented.cpu().numpy())
    out3 = meshclean.close_holes(v, _dev(flipped), max_edges=64)
    np.testing.assert_array_equal(out3.faces.cpu().numpy(), ref.close_holes(verts, flipped, max_edges=64).faces)
    same =np.sort(out3.faces[len(faces):].cpu().numpy(), 1) == np.sort(out.faces[len(faces):].cpu().numpy(), 1)
    assert same.all()                                        # the triangulation does not depend on the winding


def test_determinism_and_relabelling():
    from neuraludf_amd import meshclean
    verts, faces, _ = _case("sphere")
    a = meshclean.close_holes(_dev(verts), _dev(faces), max_edges=64)
    b = meshclean.close_holes(_dev(verts), _dev(faces), max_edges=64)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = np.random.default_rng(5).permutation(len(verts))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    info_a, info_c = {}, {}
    meshclean.close_holes(_dev(verts), _dev(faces), max_edges=64, _info=info_a)
    c = meshclean.close_holes(_dev(verts[perm]), _dev(inv[faces]), max_edges=64, _info=info_c)
    la = (info_a["loops"].loop_off[1:] - info_a["loops"].loop_off[:-1]).tolist()
    lc = (info_c["loops"].loop_off[1:] - info_c["loops"].loop_off[:-1]).tolist()
    assert len(la) == len(lc)
    assert sorted(zip(la, a.status.tolist())) == sorted(zip(lc, c.status.tolist()))
    assert c.faces.shape == a.faces.shape


def test_extract_udf_mesh_closes_holes():
    from neuraludf_amd import meshclean, meshing
    from neuraludf_amd.models import fields
    udf = build_modules(fields, seed=0)["udf"].to(DEV)
    v0, f0 = meshing.extract_udf_mesh(udf, 33)
    v1, f1 = meshing.extract_udf_mesh(udf, 33, close_holes=32)
    want = meshclean.close_holes(_dev(v0), _dev(f0), 32)
    assert v1.tobytes() == v0.tobytes() and f1.tobytes() == want.faces.cpu().numpy().tobytes()
    b0, b1 = _edges(f0, len(v0))[0], _edges(f1, len(v1))[0]
    print(f"N=33: {len(b0)} -> {len(b1)} border edges, {len(f0)} -> {len(f1)} faces, status "
          f"{torch.bincount(want.status.long()).tolist()}")
    assert len(b1) <= len(b0)
    v2, f2 = meshing.extract_udf_mesh(udf, 33, close_holes=None, close_holes_perimeter=None)
    assert v2.tobytes() == v0.tobytes() and f2.tobytes() == f0.tobytes()
    v3, f3 = meshing.extract_udf_mesh(udf, 33, fill_holes=True, close_holes=32, close_holes_perimeter=0.5, smooth_borders=True)
    filled = meshclean.fill_holes(_dev(v0), _dev(f0))[0]
    want3 = meshclean.close_holes(_dev(v0), filled, 32, 0.5).faces
    assert f3.tobytes() == want3.cpu().numpy().tobytes()
    assert v3.tobytes() == meshclean.smooth_borders(_dev(v0), want3).cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="close_holes"):
        meshing.extract_udf_mesh(udf, 33, close_holes_perimeter=1.0)


def test_cli_prints_its_lines(tmp_path, capsys):
    from neuraludf_amd import meshing
    verts, faces, _ = _case("sphere")
    meshing.write_ply(tmp_path / "in.ply", verts.astype(np.float32), faces)
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--border-loops", "--close-holes", "64"]) == 0
    text = capsys.readouterr().out
    assert "border_loops: 10 loops" in text and "loop 0: closed, " in text and " edges, perimeter " in text
    assert "close_holes: 8 of 10 loops closed (filled 8, too_many_edges 2)" in text
    rv, rf = meshing.read_ply(tmp_path / "in.ply")
    _, of = meshing.read_ply(tmp_path / "out.ply")
    np.testing.assert_array_equal(of, ref.close_holes(rv, rf, max_edges=64).faces)
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "same.ply"), "--border-loops"]) == 0
    assert "close_holes" not in capsys.readouterr().out
    np.testing.assert_array_equal(meshing.read_ply(tmp_path / "same.ply")[1], rf)
    assert meshing.main([str(tmp_path / "in.ply"), str(tmp_path / "small.ply"), "--close-holes", "7", "--close-holes-perimeter",
                         "0.2"]) == 0
    assert "close_holes: " in capsys.readouterr().out
