"""The mesh, meshing and evaluation tools may not depend on memory nobody wrote.

meshing.py, meshclean.py, meshrender.py and evaluation.py allocate their float32 / float64 outputs and scratch with
torch.empty, and each buffer has elements that only some inputs reach: pixels nothing is drawn into, vertices behind a camera
or seen by no view, clusters that are not accepted, degenerate faces, refused loops, queries beyond `bound`, rays that miss,
internal nodes of the winding tree, unselected sparse blocks.  The tools are deterministic by design (no floating-point
atomics), so the exact property of tests/scratch_poison.py applies: every case runs the clean leg (allocations filled with
0.0) twice and one leg per poison (NaN, +Inf, -1e30, 1e5) through test_gpu_scratch_poison._legs, and every tensor the call
returns or writes into `_info` must hold the SAME BITS (SP.same_bits: the results legitimately hold inf and NaN) in all
legs -- with three stated exceptions, the `rounds` counts of orient_faces, face_components and thin: they count launches of
kernels that read labels or states other threads of the same launch are changing, so the fixed point is the same in any order
and the number of rounds to it is not.  They are left out of the comparison where they are taken, held to the bounds that
are true in any order, and listed in DESIGN.md section 4.1l.  Objects with buffers of their own (MeshIndex, its winding tree, the sparse grids) are built inside the poisoned block.
Integer buffers are never poisoned; the float -> index conversions of these kernels were read first.

The clean leg is held to the operator's numpy restatement (tests/*_ref.py) with the comparison of the operator's own test
file, and the branch that leaves elements unwritten is asserted from that restatement or from returned counts, never by
looking into a poisoned buffer.

Where no fixture of the operators' own tests fits, the cases share the "hostile" mesh of tests/mesh_poison_cases.py (checked
on the CPU by tests/test_mesh_poison_cases.py).  The marching-cubes drivers run on a small sphere and a small open disc near
one corner of the box, so that the opposite block of the 2 x 2 x 2 is not selected: the two UDF drivers on both, the two
level-set drivers on the sphere's signed distance at level 0 and on the shell {udf = 0.1} of the disc."""
import functools
import math

import numpy as np
import pytest
import torch

import scratch_poison as SP
from mesh_poison_cases import FAN_VERTEX, hostile
from test_gpu_scratch_poison import _legs

pytestmark = pytest.mark.gpu

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield torch.device("cuda:0")
    torch.cuda.empty_cache()                 # poisoned float64 blocks do not stay in the allocator for later tests


def flatten(obj, name="out", out=None):
    """every tensor and number of a result (tensors, NamedTuples, tuples, dicts of them) as {name: tensor}; a number becomes
    a float64 scalar, so that a count or a length that came out of a poisoned buffer shows as well"""
    out = {} if out is None else out
    if isinstance(obj, torch.Tensor):
        out[name] = obj.detach().clone()
    elif isinstance(obj, (bool, int, float, np.integer, np.floating)):
        out[name] = torch.tensor(float(obj), dtype=torch.float64)
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            if not str(k).startswith("_"):
                flatten(obj[k], f"{name}.{k}", out)
    elif isinstance(obj, (tuple, list)) and obj and all(isinstance(v, torch.cuda.Event) for v in obj):
        pass                                     # a stage's pair of timing events (`_events` dicts): nothing to compare
    elif isinstance(obj, (tuple, list)):
        fields = getattr(obj, "_fields", None)
        for i, v in enumerate(obj):
            flatten(v, f"{name}.{fields[i] if fields else i}", out)
    elif obj is None:
        pass
    elif isinstance(obj, (str, np.ndarray)):
        if isinstance(obj, np.ndarray):
            out[name] = torch.from_numpy(np.ascontiguousarray(obj))
    else:
        raise TypeError(f"{name}: {type(obj)}")
    return out


def legs(run, dev, tag):
    clean, bad = _legs(run, dev, (), tag, differ=SP.same_bits_names, equal=SP.same_bits)
    return {k: v.cpu() for k, v in clean.items()}, bad


def _np(t):
    return t.cpu().numpy()


def _bytes_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _D(dev):
    return lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# meshrender
# ---------------------------------------------------------------------------------------------------------------------
MR_H, MR_W, MR_GAP, MR_FILL = 16, 24, 0.05, (0.1, 0.2, 0.3)


@functools.lru_cache(maxsize=None)
def render_scene():
    import meshraster_scenes as S
    v, f, _ = hostile()
    mats = np.stack([S.pinhole(20.0, 12.0, 8.0, C=(0.0, 0.0, -2.5)),           # the whole mesh, with empty pixels around it
                     S.pinhole(20.0, 2.0, 8.0, C=(0.0, 0.0, -2.5)),            # the same camera shifted: partly off-screen
                     S.pinhole(20.0, 12.0, 8.0, C=(0.0, 0.0, 2.5))])           # looks away: the whole mesh behind it
    rng = np.random.default_rng(5)
    imgs = rng.random((3, MR_H, MR_W, 3)).astype(np.float32)
    return v, f, mats, imgs


def test_rasteriser_visibility_and_colours(dev):
    """rasterize, vertex_visibility, color_vertices and normal_map over 3 views of 24 x 16 in chunks of 2 (the last chunk
    is partial)"""
    import meshraster_ref as R
    from neuraludf_amd import meshclean, meshrender
    from test_gpu_meshraster import ULP32, _same
    v, f, mats, imgs = render_scene()
    D = _D(dev)

    def run():
        dv, df = D(v), D(f)
        info = {}
        raster = meshrender.rasterize(dv, df, mats, MR_H, MR_W, view_chunk=2, _info=info)
        normals = meshclean.vertex_normals(dv, df, torch.float64)
        vis = meshrender.vertex_visibility(dv, df, mats, MR_H, MR_W, min_gap=MR_GAP, view_chunk=2)
        colors, n_seen = meshrender.color_vertices(dv, df, mats, D(imgs), normals=normals, power=2.0, min_gap=MR_GAP,
                                                   fill=MR_FILL, view_chunk=2)
        plain, n_plain = meshrender.color_vertices(dv, df, mats, D(imgs), min_gap=MR_GAP, fill=MR_FILL, view_chunk=2)
        return flatten(dict(raster=raster, info=info, normals=normals, vis=vis, colors=colors, n_seen=n_seen, plain=plain,
                            n_plain=n_plain, normal_map=meshrender.normal_map(raster, df, normals),
                            mean_edge=meshrender.mean_edge_length(dv, df),
                            mean_edge_empty=meshrender.mean_edge_length(dv, df[:0])))

    clean, bad = legs(run, dev, "meshrender")
    rinfo = {}
    want = R.rasterize(v, f, mats, MR_H, MR_W, rinfo)
    # the branches, from the restatement: empty pixels in every view, a view that draws nothing, a face partly off-screen
    assert all((want[1][i] == -1).any() for i in range(3)) and (want[1][2] == -1).all() and (want[1][0] >= 0).any()
    assert rinfo["skipped"] == len(f) and not np.isfinite(want[0][2]).any()
    scr, npix = rinfo["scr"], rinfo["npix"]
    off = (scr[1][:, 0] < 0)[f].any(1) & (npix.reshape(3, -1)[1] > 0)
    assert off.any()
    _same(tuple(_np(clean[f"out.raster.{k}"]) for k in ("depth", "face", "bary")), want)
    assert int(clean["out.info.skipped"]) == rinfo["skipped"]
    assert int(clean["out.info.small"] + clean["out.info.large"]) == int((npix > 0).sum())
    want_vis = R.visible(scr, want[0], MR_GAP)
    assert np.array_equal(_np(clean["out.vis"]), want_vis) and not want_vis[2].any() and want_vis[0].any()
    cam = R.camera_positions(mats)
    for key, nkey, nrm, power in (("out.colors", "out.n_seen", _np(clean["out.normals"]), 2.0), ("out.plain", "out.n_plain", None, 1.0)):
        ref_c, ref_n = R.colour(v, mats, want_vis, imgs, nrm, cam, power, MR_FILL)
        assert (ref_n == 0).any() and (ref_n > 0).any()                          # vertices no view sees get the fill
        assert np.array_equal(_np(clean[nkey]), ref_n) and np.abs(_np(clean[key]) - ref_c).max() <= ULP32
        assert np.array_equal(_np(clean[key])[ref_n == 0], np.tile(np.float32(MR_FILL), (int((ref_n == 0).sum()), 1)))
    assert math.isnan(float(clean["out.mean_edge_empty"]))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# meshing: the four marching-cubes drivers at 17^3 samples, block 8
# ---------------------------------------------------------------------------------------------------------------------
MC_N, MC_B, MC_LIP = 17, 8, 1.05
MC_CENTRE = (-0.8, -0.8, -0.8)          # 1.6 cells from three walls: the block at the opposite corner is > 9.01 h away


def _shift(p):
    return p - torch.tensor(MC_CENTRE, dtype=p.dtype, device=p.device)


def small_sphere_udf(p):
    import meshudf_sparse_ref as S
    return S.sphere_udf(_shift(p), radius=0.1875)


def small_disc_udf(p):
    import meshudf_sparse_ref as S
    return S.disc_udf(_shift(p), rho=0.15, c=0.0123)


def small_sphere_sdf(p):
    return _shift(p).norm(dim=-1) - 0.1875


@pytest.mark.parametrize("shape", ["sphere", "disc"])
def test_udf_marching_cubes_dense_and_sparse(dev, shape):
    import meshudf_ref as R
    import meshudf_sparse_ref as S
    from neuraludf_amd import meshing
    from neuraludf_amd.models import udf_renderer_blending as rb
    fn = dict(sphere=small_sphere_udf, disc=small_disc_udf)[shape]
    field = S.Field(fn).to(dev)
    nb = S.block_geometry(MC_N, MC_B)[0]
    blocks = S.select(S.coarse_values(fn, MC_N, MC_B, *BOX), MC_N, MC_B, S.threshold(*BOX, MC_N, MC_B, MC_LIP))
    assert 0 < len(blocks) < nb ** 3                                       # an unselected block, by the restatement
    U_ref = S.grid_values(fn, MC_N, *BOX).numpy()
    active = S.active_cells(U_ref, *BOX)
    assert active.any() and not active.all()                               # cells without a triangle

    def run():
        U, G = meshing.udf_grid(field, MC_N, *BOX)
        v, f = meshing.udf_marching_cubes(U, G, *BOX)
        g = meshing.udf_sparse_grid(field, MC_N, *BOX, block=MC_B, lipschitz=MC_LIP)
        sv, sf = meshing.udf_marching_cubes_sparse(g)
        far = U.clone()                                                    # points outside the band: G stays 0 there
        band = meshing.udf_gradients_in_band(field, far, *BOX, grad_band=1.0)
        return flatten(dict(U=U, G=G, v=v, f=f, sv=sv, sf=sf, blocks=g.blocks, slot=g.block_slot, gU=g.U, gG=g.G,
                            coarse=g.coarse, counts=(g.n_coarse, g.n_blocks, g.n_queried, g.n_grad), band=band,
                            dense=g.to_dense()))

    clean, bad = legs(run, dev, f"udf marching cubes {shape}")
    assert np.array_equal(_np(clean["out.blocks"]), blocks) and int(clean["out.counts.1"]) == len(blocks)
    h = meshing.grid_spacing(*BOX, MC_N)
    outside = _np(clean["out.U"]) >= 1.0 * h
    assert outside.any() and (~outside).any() and not _np(clean["out.band"])[outside].any()
    ax = rb._grid_axes(*BOX, MC_N, torch.device("cpu"))
    rv, rf = R.marching_cubes(_np(clean["out.U"]), _np(clean["out.G"]), _np(ax), *BOX)
    assert len(rf) > 0
    np.testing.assert_array_equal(_np(clean["out.f"]), rf)
    assert clean["out.v"].shape == rv.shape and float(np.abs(_np(clean["out.v"]) - rv).max()) <= 1e-6 * 2.0
    # the sparse mesher gives the dense mesher's mesh, order included (no active cell lies in an unselected block)
    assert S.uncovered_active_cells(U_ref, blocks, MC_B, *BOX) == 0
    assert torch.equal(clean["out.sf"], clean["out.f"]) and torch.equal(clean["out.sv"], clean["out.v"])
    assert not bad, "\n".join(bad)


# (field, level): the sphere's signed distance at level 0; an open disc has no signed field, so the shell {udf = 0.1} of its UDF
ISO_CASES = {"sphere": (small_sphere_sdf, 0.0), "disc": (lambda p: small_disc_udf(p)[0][..., 0], 0.1)}


@pytest.mark.parametrize("shape", list(ISO_CASES))
def test_iso_marching_cubes_dense_and_sparse(dev, shape):
    import isosurface_ref as R
    from neuraludf_amd import meshing
    from neuraludf_amd.models.udf_renderer_blending import extract_fields
    field, level = ISO_CASES[shape]
    nb = R.block_geometry(MC_N, MC_B)[0]
    lo, hi = R.selection_bounds(*BOX, MC_N, level, MC_B, MC_LIP)
    blocks = R.select(R.coarse_values(field, MC_N, MC_B, *BOX), MC_N, MC_B, lo, hi)
    assert 0 < len(blocks) < nb ** 3

    def run():
        F = torch.from_numpy(np.ascontiguousarray(extract_fields(BOX[0], BOX[1], MC_N, field, dev))).to(dev)
        v, f = meshing.iso_marching_cubes(F, level, *BOX)
        g = meshing.iso_sparse_grid(field, MC_N, level, *BOX, block=MC_B, lipschitz=MC_LIP, device=dev)
        sv, sf = meshing.iso_marching_cubes_sparse(g, level)
        return flatten(dict(F=F, v=v, f=f, sv=sv, sf=sf, blocks=g.blocks, slot=g.block_slot, gF=g.F, coarse=g.coarse,
                            counts=(g.n_coarse, g.n_blocks, g.n_queried)))

    clean, bad = legs(run, dev, f"iso marching cubes {shape}")
    assert np.array_equal(_np(clean["out.blocks"]), blocks)
    F = _np(clean["out.F"])
    rv, rf = R.marching_cubes(F, level, R.grid_axes(MC_N, *BOX))
    assert len(rf) > 0 and R.uncovered_cut_cells(F, level, blocks, MC_B) == 0
    np.testing.assert_array_equal(_np(clean["out.f"]), rf)
    assert clean["out.v"].shape == rv.shape and float(np.abs(_np(clean["out.v"]) - rv).max()) <= 1e-6 * 2.0
    assert torch.equal(clean["out.sf"], clean["out.f"]) and torch.equal(clean["out.sv"], clean["out.v"])
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------------------------
EV_BOUND = 0.25


@functools.lru_cache(maxsize=None)
def eval_inputs():
    v, f, _ = hostile()
    rng = np.random.default_rng(77)
    near = v[rng.integers(0, 162, 24)] * rng.uniform(0.8, 1.25, (24, 1))
    far = np.array([[0.0, 0.0, 0.0], [0.02, -0.01, 0.03], [3.0, 0.1, 0.2], [-0.1, 2.5, 0.0]])     # beyond the bound
    q = np.ascontiguousarray(np.concatenate([near, far, rng.uniform(-1.0, 1.0, (9, 3))]))
    d = rng.normal(size=(37, 3))
    o = 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    dirs = -o + rng.normal(scale=0.25, size=o.shape)
    dirs[::3] = o[::3] + rng.normal(scale=0.1, size=o[::3].shape)           # every third ray points away: a miss
    dirs[1] = v[FAN_VERTEX] * 3 - o[1]                                      # through the hole of the removed fan
    one = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], dtype=np.int64))
    return q, np.ascontiguousarray(o), np.ascontiguousarray(dirs), one


def test_mesh_index_closest_and_cast(dev):
    """MeshIndex.closest with a finite bound, .cast in its three modes, a mesh of one face, and no queries at all"""
    import meshdist_ref as RD
    import meshray_ref as RR
    from neuraludf_amd import evaluation as E
    from test_gpu_meshdist import _same as same_closest
    from test_gpu_meshray import _same as same_rays
    v, f, _ = hostile()
    q, o, d, (v1, f1) = eval_inputs()
    D = _D(dev)

    def run():
        idx = E.MeshIndex(D(v), D(f))
        single = E.MeshIndex(D(v1), D(f1))
        out = dict(closest=idx.closest(D(q), EV_BOUND), unbounded=idx.closest(D(q)), none=idx.closest(D(q[:0]), EV_BOUND),
                   single=single.closest(D(q), EV_BOUND), no_rays=idx.cast(D(o[:0]), D(d[:0])))
        for m in RR.MODES:
            out["cast " + m] = idx.cast(D(o), D(d), mode=m)
            out["single cast " + m] = single.cast(D(o), D(d), mode=m)
            out["window " + m] = idx.cast(D(o), D(d), t_min=0.5, t_max=1.9, mode=m)
        return flatten(out)

    clean, bad = legs(run, dev, "MeshIndex closest / cast")
    C = lambda name: tuple(_np(clean[f"out.{name}.{k}"]) for k in ("dist", "face", "point", "bary"))
    want = RD.closest(q, v, f, bound=EV_BOUND)
    assert (want[1] == -1).sum() >= 4 and (want[1] >= 0).sum() >= 20 and np.isinf(want[0]).any() and np.isnan(want[2]).any()
    same_closest(C("closest"), want, "bound")
    same_closest(C("unbounded"), RD.closest(q, v, f), "no bound")
    same_closest(C("single"), RD.closest(q, v1, f1, bound=EV_BOUND), "single face")
    assert clean["out.none.dist"].shape == (0,) and clean["out.none.point"].shape == (0, 3)
    for name, (mv, mf), kw in (("cast", (v, f), {}), ("single cast", (v1, f1), {}), ("window", (v, f), dict(t_min=0.5, t_max=1.9))):
        first = RR.cast(o, d, mv, mf, mode="first", **kw)
        if name != "window":
            assert (first[1] == -1).any() and np.isnan(first[2]).any()            # rays that miss
        if name == "cast":
            assert (first[1] >= 0).sum() >= 10
        same_rays(tuple(_np(clean[f"out.{name} first.{k}"]) for k in ("t", "face", "bary")), first, name + " first")
        same_rays(_np(clean[f"out.{name} any"]), RR.cast(o, d, mv, mf, mode="any", **kw), name + " any")
        same_rays(_np(clean[f"out.{name} count"]), RR.cast(o, d, mv, mf, mode="count", **kw), name + " count")
    assert not bad, "\n".join(bad)


def test_mesh_index_winding_and_intersections(dev):
    import meshintersect_ref as RI
    import meshwinding_ref as RW
    from neuraludf_amd import evaluation as E
    from test_gpu_meshwinding import _check
    v, f, _ = hostile()
    q = eval_inputs()[0]
    v2 = v + np.array([0.3, 0.05, -0.02])
    D = _D(dev)
    made = {}

    def run():
        idx = E.MeshIndex(D(v), D(f))
        out = dict(winding=idx.winding(D(q), _counts=True), exact=idx.winding(D(q), beta=math.inf, _counts=True),
                   none=idx.winding(D(q[:0])), self_isect=idx.intersections(), other=idx.intersections((D(v2), D(f))))
        tree = idx._winding_tree
        made.setdefault("leaf", tree.leaf)                                 # (the first leg is a clean one)
        out["tree"] = dict(rec=tree.rec, first=tree.first, count=tree.count, skip=tree.skip, level=tree.level, faces=tree.faces)
        return flatten(out)

    clean, bad = legs(run, dev, "MeshIndex winding / intersections")
    ref = RW.Tree(v, f, leaf=made["leaf"])
    assert int((~ref.is_leaf).sum()) >= 1                                         # internal nodes: records summed from below
    assert clean["out.tree.rec"].shape == (ref.n_nodes, 32) and _np(clean["out.tree.rec"]).tobytes() == ref.rec.tobytes()
    for name, beta in (("winding", 2.0), ("exact", math.inf)):
        want = RW.winding(ref, q, beta)
        _check(tuple(_np(clean[f"out.{name}.{i}"]) for i in range(3)), want)
    assert (RW.winding(ref, q, 2.0)["far"] > 0).any()
    # (the restatement takes the querying mesh first and the indexed one as `other`)
    for name, want in (("self_isect", RI.pairs(v, f)), ("other", RI.pairs(v2, f, other=(v, f)))):
        got = [(a, b, k) for (a, b), k in zip(clean[f"out.{name}.pairs"].tolist(), clean[f"out.{name}.kind"].tolist())]
        assert got == want, name
        assert (len(want) > 10) == (name == "other")
    assert not bad, "\n".join(bad)


def test_point_cloud_tools(dev):
    """nearest with a bound, thin, sample_mesh and mesh_deviation"""
    import pointcloud_ref as RP
    from neuraludf_amd import evaluation as E
    v, f, _ = hostile()
    q = eval_inputs()[0]
    v2 = v * np.array([1.05, 0.97, 1.0]) + 0.01
    D = _D(dev)
    rounds = []

    def run():
        info, ev = {}, {}
        pts = E.sample_mesh(D(v), D(f), 0.05)
        # NOT COMPARED: thin's round count.  A round reads the states of lower-ranked points in place while other threads of
        # the same launch decide them (pc_thin_round_kernel): each decision is the sequential one whatever the order, the
        # number of rounds it takes is not.  The mask is compared.
        keep = E.thin(pts, 0.08, _info=info)
        rounds.append(info["rounds"])
        out = dict(pts=pts, nearest=E.nearest(D(q), D(v), EV_BOUND, _events=ev), nearest_events={k: ev[k] for k in ("cell", "cells")},
                   none=E.nearest(D(q[:0]), D(v), EV_BOUND), thin=keep,
                   deviation=E.mesh_deviation((D(v), D(f)), (D(v2), D(f)), density=0.05, bound=EV_BOUND),
                   unbounded=E.mesh_deviation((D(v), D(f)), (D(v2), D(f)), density=0.05))
        return flatten(out)

    clean, bad = legs(run, dev, "point cloud tools")
    assert {"out.nearest_events.cell", "out.nearest_events.cells"} <= set(clean)
    want_pts = RP.sample_mesh(v, f, 0.05)
    _bytes_equal(_np(clean["out.pts"]), want_pts, "sample_mesh")
    assert len(want_pts) > len(v) + 500
    dist, idx = RP.nearest(q, v, EV_BOUND)
    assert (idx == -1).any() and (idx >= 0).any() and np.isinf(dist).any()                # queries beyond the bound
    _bytes_equal(_np(clean["out.nearest.0"]), dist, "nearest dist")
    _bytes_equal(_np(clean["out.nearest.1"]), idx, "nearest idx")
    keep = RP.thin(want_pts, 0.08)
    assert 0 < keep.sum() < len(keep)
    assert len(rounds) == 6 and all(1 <= r <= len(keep) for r in rounds), rounds      # (thin raises beyond one round per point)
    _bytes_equal(_np(clean["out.thin"]), keep, "thin")
    # mesh_deviation: the sampled clouds against the other mesh, by the restatements of its two halves
    import meshdist_ref as RD
    sides = dict(a_to_b=RD.closest(want_pts, v2, f)[0], b_to_a=RD.closest(RP.sample_mesh(v2, f, 0.05), v, f)[0])
    for side, d in sides.items():
        assert float(clean[f"out.unbounded.{side}.max"]) == d.max() and int(clean[f"out.unbounded.{side}.n"]) == len(d)
        assert abs(float(clean[f"out.unbounded.{side}.mean"]) - d.mean()) <= 1e-12 * d.mean()
        assert abs(float(clean[f"out.unbounded.{side}.rms"]) - math.sqrt((d * d).mean())) <= 1e-12 * d.max()
    assert float(clean["out.unbounded.hausdorff"]) == max(d.max() for d in sides.values()) > EV_BOUND
    assert float(clean["out.deviation.hausdorff"]) == math.inf                       # samples beyond the bound
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# meshclean
# ---------------------------------------------------------------------------------------------------------------------
def _attributes(v):
    return np.ascontiguousarray(np.stack([np.sin(3.0 * v[:, 0]), v[:, 1] * v[:, 2], 0.5 + 0.0 * v[:, 0]], 1))


def test_holes_borders_orientation_and_components(dev):
    import meshclean_ref as RC
    import meshhole_ref as RH
    import meshorient_ref as RO
    from neuraludf_amd import meshclean as M
    v, f, parts = hostile()
    rng = np.random.default_rng(3)
    scrambled = np.where((rng.random(len(f)) < 0.4)[:, None], f[:, [0, 2, 1]], f)
    D = _D(dev)
    rounds = []

    def run():
        dv = D(v)
        info, oinfo, cinfo = {}, {}, {}
        closed = M.close_holes(dv, D(f), max_edges=32, _info=info)
        orient = M.orient_faces(dv, D(scrambled), outward_from=(0.0, 0.0, 0.0), _info=oinfo)
        labels = M.face_components(D(f), len(v), _info=cinfo)
        # NOT COMPARED: the two `rounds` counts.  The hook kernels of both union-finds (mo_hook_kernel, mt_cc_hook_kernel)
        # walk to the roots through labels that other threads lower with atomicMin in the same launch: the labels reach the
        # same fixed point whatever the order, the number of launches it takes does not.  They differ from run to run with
        # nothing poisoned (DESIGN.md section 4.1l lists them); every other entry of the two dicts is compared.
        rounds.append((oinfo.pop("rounds"), cinfo.pop("rounds")))
        return flatten(dict(closed=closed, loops=info["loops"], borders=M.border_loops(dv, D(f)),
                            tight=M.close_holes(dv, D(f), max_edges=32, max_perimeter=0.2), orient=orient, oinfo=oinfo,
                            plain=M.orient_faces(dv, D(scrambled)), normals=M.vertex_normals(dv, orient.faces, torch.float64),
                            normals32=M.vertex_normals(dv, orient.faces), labels=labels,
                            cinfo=cinfo, kept=M.filter_components(dv, D(f), min_faces=3),
                            largest=M.filter_components(dv, D(f), keep_largest=True)))

    clean, bad = legs(run, dev, "holes, borders, orientation, components")
    # what holds of the round counts in any order: at least one round (there are manifold edges), and no more than the
    # drivers allow before they raise (every round that changes something lowers a parent)
    assert len(rounds) == 6 and all(1 <= r <= len(f) + 1 for pair in rounds for r in pair), rounds
    assert set(clean) >= {"out.oinfo.components", "out.oinfo.flipped", "out.oinfo.orientable", "out.oinfo.non_orientable"}
    want_o = RO.orient(v, scrambled, (0.0, 0.0, 0.0))
    assert int(clean["out.oinfo.components"]) == len(np.unique(want_o[2])) == 3
    assert int(clean["out.oinfo.flipped"]) == int(want_o[1].sum()) and int(clean["out.oinfo.non_orientable"]) == 0
    want = RH.close_holes(v, f, max_edges=32)
    assert (want.status == RH.FILLED).sum() == 1 and (want.status != RH.FILLED).sum() == 2           # refused loops
    np.testing.assert_array_equal(_np(clean["out.closed.faces"]), want.faces)
    np.testing.assert_array_equal(_np(clean["out.closed.new_face_loop"]), want.new_face_loop)
    np.testing.assert_array_equal(_np(clean["out.closed.status"]), want.status)
    tight = RH.close_holes(v, f, max_edges=32, max_perimeter=0.2)
    assert (tight.status == RH.PERIMETER).any()                                                     # refused for its length
    np.testing.assert_array_equal(_np(clean["out.tight.status"]), tight.status)
    np.testing.assert_array_equal(_np(clean["out.tight.faces"]), tight.faces)
    tb = RH.table(f, len(v))
    lp = RH.loops(tb, RH.link(f, tb))
    per = RH.count(v, tb, lp, 64)[0]
    assert _np(clean["out.borders.perimeter"]).tobytes() == per.tobytes() == _np(clean["out.loops.perimeter"]).tobytes()
    np.testing.assert_array_equal(_np(clean["out.borders.loop_vertex"]), lp.loop_vertex)
    for key, origin in (("orient", (0.0, 0.0, 0.0)), ("plain", None)):
        for got, w, name in zip((clean[f"out.{key}.{k}"] for k in ("faces", "flipped", "labels", "orientable")),
                                RO.orient(v, scrambled, origin), ("faces", "flipped", "labels", "orientable")):
            np.testing.assert_array_equal(_np(got), w, err_msg=f"{key} {name}")
    wn = RO.vertex_normals(v, _np(clean["out.orient.faces"]))
    assert not wn[list(parts["unreferenced"])].any() and np.abs(_np(clean["out.normals"]) - wn).max() <= 1e-12
    np.testing.assert_array_equal(_np(clean["out.normals32"]), _np(clean["out.normals"]).astype(np.float32))
    np.testing.assert_array_equal(_np(clean["out.labels"]), RC.face_components(f, len(v)))
    for key, kw in (("kept", dict(min_faces=3)), ("largest", dict(keep_largest=True))):
        wv, wf = RC.filter_components(v, f, **kw)
        assert len(wf) < len(f)
        np.testing.assert_array_equal(_np(clean[f"out.{key}.0"]), wv)
        np.testing.assert_array_equal(_np(clean[f"out.{key}.1"]), wf)
    assert not bad, "\n".join(bad)


def test_smoothing_and_denoising(dev):
    import meshsmooth_ref as RS
    from neuraludf_amd import meshclean as M
    from test_gpu_meshsmooth import CAP
    v, f, parts = hostile()
    mask = np.random.default_rng(4).random(len(v)) < 0.2
    D = _D(dev)

    def run():
        dv, df = D(v), D(f)
        return flatten(dict(uniform=M.smooth_mesh(dv, df, 3), cotangent=M.smooth_mesh(dv, df, 3, weights="cotangent"),
                            free=M.smooth_mesh(dv, df, 2, weights="cotangent", boundary="free", fixed=D(mask)),
                            f32=M.smooth_mesh(dv.float(), df, 3), denoise=M.denoise_mesh(dv, df, 2, 3),
                            no_normal_steps=M.denoise_mesh(dv, df, 0, 2, boundary="free")))

    clean, bad = legs(run, dev, "smoothing and denoising")
    area = RS.frames(v, f)[1]
    assert (area == 0).sum() == 1 and len(RS.border_vertices(f, len(v))) > 0            # the zero-area face, border vertices
    np.testing.assert_array_equal(_np(clean["out.uniform"]), RS.smooth_mesh(v, f, 3))
    np.testing.assert_array_equal(_np(clean["out.cotangent"]), RS.smooth_mesh(v, f, 3, weights="cotangent"))
    np.testing.assert_array_equal(_np(clean["out.free"]), RS.smooth_mesh(v, f, 2, weights="cotangent", boundary="free", fixed=mask))
    np.testing.assert_array_equal(_np(clean["out.uniform"])[list(parts["unreferenced"])], v[list(parts["unreferenced"])])
    for key, args, kw in (("denoise", (2, 3), {}), ("no_normal_steps", (0, 2), dict(boundary="free"))):
        pos, fn = RS.denoise_mesh(v, f, *args, **kw)
        assert not fn[parts["zero_area"]].any()
        assert np.abs(_np(clean[f"out.{key}.0"]) - pos).max() <= CAP and np.abs(_np(clean[f"out.{key}.1"]) - fn).max() <= CAP
    assert not bad, "\n".join(bad)


def test_simplify_and_transfer(dev):
    import meshsimplify_ref as RS
    import meshremesh_ref as RR
    from neuraludf_amd import meshclean as M
    from test_gpu_meshsimplify import _assert_matches
    v, f, parts = hostile()
    attr = _attributes(v)
    cell = 0.37                          # chosen on the restatement: two clusters are not accepted, one is dropped
    origin = RS.lowered_origin(v, cell)
    dst = eval_inputs()[0]
    D = _D(dev)
    made = {}

    def run():
        info = {}
        got = M.simplify_mesh(D(v), D(f), cell, origin=tuple(origin), attributes=D(attr), _info=info)
        made.setdefault("got", got), made.setdefault("info", info)        # the first leg is a clean one
        return flatten(dict(simplified=got, info=info, mean=M.simplify_mesh(D(v), D(f), cell, origin=tuple(origin), placement="mean"),
                            transfer=M.transfer_attributes(D(v), D(f), D(attr), D(dst), bound=EV_BOUND),
                            transfer_all=M.transfer_attributes(D(v), D(f), D(attr), D(dst))))

    clean, bad = legs(run, dev, "simplify and transfer")
    want = RS.simplify(v, f, cell, origin=origin, attributes=attr)
    assert (~want.accepted).any() and want.accepted.any() and (want.vertex_cluster == -1).any()      # rejected and dropped clusters
    assert want.wall_margin > 1e-6
    _assert_matches(made["got"], made["info"], want, cell)
    assert int(clean["out.info.fallbacks"]) == int((~want.accepted).sum())
    import meshdist_ref as RD
    face = RD.closest(dst, v, f, bound=EV_BOUND)[1]
    got = _np(clean["out.transfer"])
    assert (face == -1).any() and np.isnan(got[face == -1]).all() and np.isfinite(got[face >= 0]).all()
    np.testing.assert_array_equal(_np(clean["out.transfer_all"]), RR.transfer(v, f, attr, dst))
    np.testing.assert_array_equal(got[face >= 0], RR.transfer(v, f, attr, dst)[face >= 0])
    assert not bad, "\n".join(bad)


def test_subdivision_and_remeshing(dev):
    import meshremesh_ref as RR
    import meshsubdiv_ref as RS
    from neuraludf_amd import meshclean as M
    from test_gpu_meshremesh import _same as same_remesh
    from test_gpu_meshsubdiv import _same as same_subdiv
    v, f, parts = hostile()
    attr = _attributes(v)
    D = _D(dev)
    made = {}

    def run():
        dv, df, da = D(v), D(f), D(attr)
        i1, i2, i3 = {}, {}, {}
        out = dict(loop=M.subdivide_mesh(dv, df, 1, "loop", attributes=da, _info=i1), midpoint=M.subdivide_mesh(dv, df, 2, "midpoint"),
                   to_edge=M.subdivide_to_edge(dv, df, 0.12, attributes=da, _info=i2),
                   remesh=M.remesh_isotropic(dv, df, 0.2, iterations=2, project=True, attributes=da, _info=i3))
        if not made:                                                       # the first leg is a clean one
            made.update(out)
        return flatten(dict(out, i1=i1, i2=i2, i3=i3))

    clean, bad = legs(run, dev, "subdivision and remeshing")
    t = RS.edge_table(f, len(v))
    assert (np.asarray(t.count) == 1).any()                                              # border edges, so border vertices
    same_subdiv(made["loop"], RS.subdivide_mesh(v, f, 1, "loop", attributes=attr))
    same_subdiv(made["midpoint"], RS.subdivide_mesh(v, f, 2, "midpoint"))
    want = RS.subdivide_to_edge(v, f, 0.12, attributes=attr)
    assert want.rounds >= 1 and len(want.faces) > len(f)
    same_subdiv(made["to_edge"], want)
    same_remesh(made["remesh"], RR.remesh_isotropic(v, f, 0.2, iterations=2, project=True, attributes=attr))
    assert not bad, "\n".join(bad)
