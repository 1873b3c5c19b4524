"""GPU: rays against meshes (neuraludf_amd/evaluation.py MeshIndex.cast / cast_rays / contains_points / signed_distance,
csrc/meshray.hip) against the numpy restatement (tests/meshray_ref.py) bit for bit, in all three modes; the walk through
the cells probed with rays built from the index's own planes; independence of the cell size, the ray order and the run;
the layers above the kernel; the rasteriser on a shared view; Trainer.render_image(mesh=...).  What it replaces:
trimesh.ray and trimesh.Trimesh.contains on the CPU."""
import math

import numpy as np
import pytest
import torch

import meshray_ref as R
import meshsimplify_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _hand_back_the_cache():
    """float64 geometry must not stay in the blocks torch's allocator keeps for later tests' torch.empty buffers"""
    yield
    torch.cuda.empty_cache()


def _E():
    from neuraludf_amd import evaluation
    return evaluation


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _same(got, want, what=""):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            rows = np.unique(np.argwhere(np.atleast_1d(g != w) & ~(np.isnan(g) & np.isnan(w)))[:, 0])[:5]
            raise AssertionError((what, k, rows.tolist(), g[rows].tolist(), w[rows].tolist()))


def _all_modes(index, o, d, **kw):
    do, dd = _dev(o), _dev(d)
    kw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return {m: index.cast(do, dd, mode=m, **kw) for m in R.MODES}


def _want(o, d, v, f, **kw):
    return {m: R.cast(o, d, v, f, mode=m, **kw) for m in R.MODES}


def _check(got, want, what):
    _same(tuple(got["first"]), want["first"], what + ", first")
    _same(got["any"], want["any"], what + ", any")
    _same(got["count"], want["count"], what + ", count")


# ---- 1. the mixed mesh -------------------------------------------------------------------------------------------------
def _mobius(n=24, radius=0.35, half_width=0.12, centre=(0.0, 0.0, -0.85)):
    u = np.arange(n) * (2 * np.pi / n)
    rows = []
    for s in (-half_width, half_width):
        r = radius + s * np.cos(u / 2)
        rows.append(np.stack([r * np.cos(u), r * np.sin(u), s * np.sin(u / 2)], -1) + np.array(centre))
    v = np.concatenate(rows)                                   # [2 n, 3]: row 0 the inner rim, row 1 the outer
    f = []
    for i in range(n):
        j = (i + 1) % n
        a, b = i, n + i
        c, d = (j, n + j) if j else (n, 0)                     # the band closes with the rims exchanged
        f += [[a, b, d], [a, d, c]]
    return v, np.array(f, dtype=np.int64)


def _mixed_mesh():
    parts_v, parts_f = [], []

    def add(v, f):
        base = sum(len(p) for p in parts_v)
        parts_v.append(np.asarray(v, dtype=np.float64))
        parts_f.append(np.asarray(f, dtype=np.int64) + base)

    add(*R.icosphere(2, 0.6))                                                          # closed and coarse: 320 faces
    sv, sf = S.sheet(8, -0.9, -0.3)
    add(sv + np.array([0.0, 0.0, 0.8]), sf)                                            # an open sheet
    add(*R.folded_sheet())                                                             # crossed several times by one ray
    add(*_mobius())
    add([[0.7, 0.7, 0.7], [0.9, 0.8, 0.75], [0.8, 0.95, 0.7], [0.75, 0.7, 0.95], [0.9, 0.6, 0.6]],
        [[0, 1, 2], [1, 0, 3], [0, 1, 4]])                                             # three faces on one edge
    add([[-0.8, 0.7, -0.5], [-0.6, 0.8, -0.4], [-0.4, 0.9, -0.3], [-0.7, 0.5, -0.7]],
        [[0, 0, 1], [3, 3, 3], [0, 1, 2], [2, 0, 1]])                                  # repeated vertices, collinear
    add([[np.nan, 0.1, 0.2], [0.8, -0.8, 0.8], [0.9, -0.7, 0.8]], [[0, 1, 2]])         # a NaN vertex
    add([[5.0, 5.0, 5.0], [-0.95, -0.95, 0.95]], np.zeros((0, 3)))                     # unused vertices
    v, f = np.concatenate(parts_v), np.concatenate(parts_f)
    f = np.concatenate([f, f[100:101], f[-6:-5]])                                      # duplicated faces
    return v, f


def _mixed_rays(v, f, rng):
    """2 000 rays -> (o, d, t_min [N], t_max [N]): the per-ray windows; the scalar-window calls use (0, inf)"""
    ok = R.usable_faces(v, f)
    fu = f[ok]

    def unit(x):
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    def surface(n):
        t = fu[rng.integers(0, len(fu), n)]
        w = rng.dirichlet((1.0, 1.0, 1.0), n)
        return (w[:, :, None] * v[t]).sum(1)
    inside_o = rng.uniform(-1.0, 1.0, (600, 3))                                         # origins inside the grid
    inside_d = rng.normal(size=(600, 3)) * rng.uniform(0.2, 3.0, (600, 1))
    out_o = 4.0 * unit(rng.normal(size=(500, 3)))                                       # outside, aimed at the mesh
    out_d = (rng.uniform(-0.9, 0.9, (500, 3)) - out_o) * rng.uniform(0.3, 2.0, (500, 1))
    miss_o = 4.0 * unit(rng.normal(size=(200, 3)))                                      # outside, missing the box
    miss_d = np.cross(miss_o, rng.normal(size=(200, 3)))
    away_o = 3.0 * unit(rng.normal(size=(100, 3)))                                      # the box lies behind the origin
    away_d = away_o * rng.uniform(0.5, 2.0, (100, 1))
    vu = v[np.unique(fu)]
    surf_o = np.concatenate([surface(300), vu[rng.integers(0, len(vu), 100)]])          # starting on the surface, 100 at
    surf_d = rng.normal(size=(400, 3))                                                  # vertices: t = 0 exactly
    vert_o = 2.5 * unit(rng.normal(size=(200, 3)))                                      # aimed at vertices and edge points
    e = fu[rng.integers(0, len(fu), 100)]
    vert_target = np.concatenate([vu[rng.integers(0, len(vu), 100)], 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
    vert_d = vert_target - vert_o
    o = np.concatenate([inside_o, out_o, miss_o, away_o, surf_o, vert_o])
    d = np.concatenate([inside_d, out_d, miss_d, away_d, surf_d, vert_d])
    p = rng.permutation(len(o))
    o, d = o[p], d[p]
    # the per-ray windows: a t_max between the first two hits, a t_min beyond the first, whole lines, empty reaches
    t1 = R.cast(o, d, v, f)[0]
    t2 = R.cast(o, d, v, f, t_min=np.where(np.isfinite(t1), np.nextafter(t1, np.inf), 0.0))[0]
    kind = rng.integers(0, 5, len(o))
    two = np.isfinite(t2)
    t_min, t_max = np.zeros(len(o)), np.full(len(o), np.inf)
    cut = two & (kind == 0)
    t_max[cut] = 0.5 * (t1 + t2)[cut]
    skip = two & (kind == 1)
    t_min[skip] = 0.5 * (t1 + t2)[skip]
    t_min[kind == 2] = -np.inf                                                          # the whole line
    t_min[kind == 3], t_max[kind == 3] = 1e-3, 0.75
    exact = np.isfinite(t1) & (kind == 4)                                               # windows that end on a hit exactly
    t_max[exact] = t1[exact]
    return o, d, t_min, t_max


@pytest.fixture(scope="module")
def mixed():
    """the mixed mesh, its rays and the restatement's answers, computed once and left unchanged"""
    rng = np.random.default_rng(31)
    v, f = _mixed_mesh()
    o, d, t_min, t_max = _mixed_rays(v, f, rng)
    want = dict(plain=_want(o, d, v, f), positive=_want(o, d, v, f, t_min=1e-3),
                per_ray=_want(o, d, v, f, t_min=t_min, t_max=t_max))
    for a in (v, f, o, d, t_min, t_max):
        a.setflags(write=False)
    return v, f, o, d, t_min, t_max, want


def test_mixed_mesh_equals_the_restatement_bit_for_bit(mixed):
    v, f, o, d, t_min, t_max, want = mixed
    E = _E()
    assert 600 <= len(f) <= 800 and len(o) == 2000
    index = E.MeshIndex(_dev(v), _dev(f))
    got = _all_modes(index, o, d)
    _check(got, want["plain"], "t_min = 0")
    t, face, bary = want["plain"]["first"]
    assert 700 <= (face >= 0).sum() <= 1600 and (t == 0).sum() >= 80          # rays that start on the surface hit it at 0
    assert want["plain"]["count"].max() >= 4 and len(f) - 3 not in face         # the NaN face is absent
    _check(_all_modes(index, o, d, t_min=1e-3), want["positive"], "t_min > 0")
    assert (want["positive"]["first"][0] != t).sum() >= 50
    _check(_all_modes(index, o, d, t_min=t_min, t_max=t_max), want["per_ray"], "a window per ray")
    assert (want["per_ray"]["first"][1] != face).sum() >= 100
    # the same through cast_rays, from float32 rays (widened exactly), and on an empty batch
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    _same(tuple(E.cast_rays(_dev(o32), _dev(d32), _dev(v), _dev(f))),
          R.cast(o32.astype(np.float64), d32.astype(np.float64), v, f), "float32 rays")
    none = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    empty = index.cast(none, none)
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0, 3)] and empty.face.dtype == torch.int64
    assert index.cast(none, none, mode="any").dtype == torch.bool and index.cast(none, none, mode="count").dtype == torch.int64


def test_mode_consistency(mixed):
    v, f, o, d, t_min, t_max, want = mixed
    index = _E().MeshIndex(_dev(v), _dev(f))
    for kw in (dict(), dict(t_min=t_min, t_max=t_max)):
        got = _all_modes(index, o, d, **kw)
        hit = torch.isfinite(got["first"].t)
        assert torch.equal(got["any"], hit) and torch.equal(hit, got["first"].face >= 0)
        # a face hit with three non-zero weights is crossed under the counting rule too (the signs are the weights');
        # on an exactly zero edge function the counting rule gives the crossing to one side of the edge, which at a
        # border edge or at a vertex (a ray that starts at one: the 100 of _mixed_rays) can be a side with no face
        strict = hit & (got["first"].bary != 0).all(1)
        assert bool((got["count"][strict] >= 1).all()) and int(strict.sum()) >= 0.8 * int(hit.sum())
        assert bool(((got["first"].bary == 0).any(1) | ~hit | (got["count"] >= 1)).all())
        assert bool(torch.isnan(got["first"].bary[~hit]).all()) and bool((got["first"].t[~hit] == math.inf).all())
    _same(got["count"], want["per_ray"]["count"], "count")


def test_refusals():
    E = _E()
    v, f = R.cube()
    index = E.MeshIndex(_dev(v), _dev(f))
    o, d = np.zeros((2, 3)), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            index.cast(_dev(np.array([[0.0, bad, 0.0]] * 2)), _dev(d))
        with pytest.raises(ValueError, match="non-finite"):
            index.cast(_dev(o), _dev(np.array([[1.0, bad, 0.0]] * 2)))
    with pytest.raises(ValueError, match="zero"):
        index.cast(_dev(o), _dev(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])))
    with pytest.raises(ValueError, match="mode"):
        index.cast(_dev(o), _dev(d), mode="all")
    with pytest.raises(ValueError, match="t_min"):
        index.cast(_dev(o), _dev(d), t_min=1.0, t_max=0.5)
    with pytest.raises(ValueError, match="t_min"):
        index.cast(_dev(o), _dev(d), t_min=math.nan)
    with pytest.raises(ValueError, match="t_min"):
        index.cast(_dev(o), _dev(d), t_max=_dev(np.array([1.0, -1.0])))
    with pytest.raises(ValueError, match="shape"):
        index.cast(_dev(o), _dev(d[:1]))
    with pytest.raises(ValueError):
        E.cast_rays(_dev(o), _dev(d), _dev(v), _dev(f), index=index)
    with pytest.raises(ValueError):
        E.cast_rays(_dev(o), _dev(d))


# ---- 2. rays that try the walk -----------------------------------------------------------------------------------------------
def _adversarial_rays(lo, cell, grid, rng):
    """rays built from the grid's own planes lo + k cell: in cell walls, along cell edges, through cell corners, from
    origins on the planes, with one or two zero components and with tied dominant axes"""
    lo, g = np.asarray(lo), np.asarray(grid)
    o, d = [], []

    def plane(axis, k):
        return lo[axis] + k * cell
    for axis in range(3):                                   # axis-parallel rays lying exactly in a cell wall
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for k in range(0, g[a] + 1):
            for s in (1.0, -1.0):
                p = np.empty(3)
                p[axis] = lo[axis] - s * (0.7 * cell) if s > 0 else lo[axis] + (g[axis] + 0.7) * cell
                p[a] = plane(a, k)
                p[b] = lo[b] + rng.uniform(0, g[b]) * cell
                e = np.zeros(3)
                e[axis] = s * rng.uniform(0.5, 2.0)
                o.append(p), d.append(e)
        for k in range(0, g[a] + 1, 2):                     # along cell edges: two coordinates on planes
            for l in range(0, g[b] + 1, 2):
                p = np.empty(3)
                p[axis], p[a], p[b] = lo[axis] - 0.3 * cell, plane(a, k), plane(b, l)
                e = np.zeros(3)
                e[axis] = 1.0
                o.append(p), d.append(e)
                q = p.copy()                                # and from an origin inside the grid, on three planes
                q[axis] = plane(axis, min(k, g[axis]))
                o.append(q), d.append(-e)
    diag = [(1.0, 1.0, 1.0), (1.0, -1.0, 1.0), (-1.0, 1.0, 1.0), (1.0, 1.0, -1.0), (1.0, 1.0, 0.0), (0.0, 1.0, -1.0),
            (1.0, 0.0, 1.0), (-1.0, -1.0, 0.0), (2.0, 1.0, 2.0), (1.0, 2.0, -2.0)]
    for e in diag:                                          # through corner after corner; the dominant axis ties
        for _ in range(12):
            c = np.array([rng.integers(0, n + 1) for n in g])
            p = lo + c * cell
            back = rng.integers(0, 2 * max(g))
            o.append(p - back * cell * np.array(e)), d.append(np.array(e) * rng.choice([0.5, 1.0, cell, 3.0]))
    for _ in range(150):                                    # origins exactly on grid planes, generic directions
        c = np.array([rng.integers(0, n + 1) for n in g])
        p = lo + (c + rng.uniform(0, 1, 3) * (rng.uniform(size=3) < 0.5)) * cell
        o.append(p), d.append(rng.normal(size=3))
    for _ in range(150):                                    # one or two zero components, from outside and inside
        p = lo + rng.uniform(-1.0, g + 1.0) * cell
        e = rng.normal(size=3)
        e[rng.integers(0, 3)] = 0.0
        if rng.uniform() < 0.4:
            e[rng.integers(0, 3)] = 0.0
        if not e.any():
            e[0] = 1.0
        o.append(p), d.append(e)
    for _ in range(100):                                    # tied dominant axes with a generic third component
        p = lo + rng.uniform(-1.0, g + 1.0) * cell
        m = rng.uniform(0.5, 2.0)
        e = np.array([m, -m, rng.uniform(-m, m)])[rng.permutation(3)]
        o.append(p), d.append(e)
    return np.array(o), np.array(d)


def test_rays_in_walls_through_corners_and_along_edges(mixed):
    v, f = mixed[0], mixed[1]
    E = _E()
    rng = np.random.default_rng(32)
    index = E.MeshIndex(_dev(v), _dev(f))
    for factor in (1.0, 0.5, 0.25):
        idx = index if factor == 1.0 else E.MeshIndex(_dev(v), _dev(f), cell=factor * index.cell)
        o, d = _adversarial_rays(idx.lo, idx.cell, idx.grid, rng)
        assert 600 <= len(o) <= 4000
        want = _want(o, d, v, f)
        assert (want["first"][1] >= 0).sum() >= 50
        _check(_all_modes(idx, o, d), want, f"cell {idx.cell}")
        _check(_all_modes(index, o, d), want, f"rays of cell {idx.cell} on the default index")
    # a mesh whose faces lie in the walls themselves: the unit sheet in a grid of cell 1 / 8 with its origin on the sheet
    sv, sf = R.grid_sheet(8)
    idx = E.MeshIndex(_dev(sv), _dev(sf), cell=0.125)
    assert idx.cell == 0.125 and idx.lo == [0.0, 0.0, 0.0]
    o, d = _adversarial_rays(idx.lo, idx.cell, idx.grid, rng)
    down = np.concatenate([sv + np.array([0.0, 0.0, 0.5]), sv + np.array([0.25, 0.125, 0.25])])
    o = np.concatenate([o, down])
    d = np.concatenate([d, np.broadcast_to([0.0, 0.0, -1.0], sv.shape), np.broadcast_to([-1.0, -0.5, -1.0], sv.shape)])
    want = _want(o, d, sv, sf)
    assert want["first"][1][-2 * len(sv):].min() >= 0                            # every vertex is hit: nothing leaks
    _check(_all_modes(idx, o, d), want, "the sheet in the walls")


# ---- 3. independence ---------------------------------------------------------------------------------------------------------
def test_independent_of_cell_size_ray_order_and_run(mixed):
    v, f, o, d, t_min, t_max, want = mixed
    E = _E()
    base = E.MeshIndex(_dev(v), _dev(f))
    for factor in (0.5, 1.0, 3.0, 7.0):
        idx = E.MeshIndex(_dev(v), _dev(f), cell=factor * base.cell)
        assert idx.cell == factor * base.cell
        _check(_all_modes(idx, o, d, t_min=t_min, t_max=t_max), want["per_ray"], f"cell x {factor}")
    fine = E.MeshIndex(_dev(v), _dev(f), cell=base.cell / 4)
    forced = E.MeshIndex(_dev(v), _dev(f), cell=base.cell / 4, max_refs=fine.n_refs // 2)
    assert forced.cell >= 2 * fine.cell and forced.n_refs <= fine.n_refs // 2
    _check(_all_modes(forced, o, d), want["plain"], "max_refs doubles the cell")
    _check(_all_modes(fine, o, d), want["plain"], "cell / 4")
    p = np.random.default_rng(33).permutation(len(o))
    got = _all_modes(base, o[p], d[p], t_min=t_min[p], t_max=t_max[p])
    _check(got, {m: tuple(a[p] for a in w) if isinstance(w, tuple) else w[p] for m, w in want["per_ray"].items()},
           "permuted rays")
    again = _all_modes(base, o[p], d[p], t_min=t_min[p], t_max=t_max[p])
    for m in R.MODES:
        _same(tuple(again[m]) if m == "first" else again[m],
              tuple(x.cpu().numpy() for x in got[m]) if m == "first" else got[m].cpu().numpy(), "second run")


# ---- 4. the layers above the kernel ------------------------------------------------------------------------------------------
def test_contains_points_and_signed_distance():
    E = _E()
    rng = np.random.default_rng(34)
    p = rng.uniform(-0.8, 0.8, (3000, 3))
    for name in ("cube", "sphere"):
        if name == "cube":
            v, f = R.cube()
            depth = 0.5 - np.abs(p).max(1)                                      # > 0 inside
        else:
            v, f = R.icosphere(2, 0.7)
            n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            depth = (-((p[:, None, :] - v[f[:, 0]][None]) * n[None]).sum(-1)).min(1)      # convex: the exact inside test
        away = np.abs(depth) >= 1e-6
        assert away.sum() >= 2990 and (depth > 0).sum() > 500 and (depth < 0).sum() > 500
        index = E.MeshIndex(_dev(v), _dev(f))
        inside = E.contains_points(_dev(p), index)
        assert inside.dtype == torch.bool and np.array_equal(inside.cpu().numpy()[away], (depth > 0)[away])
        _same(inside, R.parity_inside(p, v, f, E.INSIDE_DIRECTIONS), name)
        sd = E.signed_distance(_dev(p), (_dev(v), _dev(f)))
        dist = E.closest_on_mesh(_dev(p), index=index).dist
        assert torch.equal(sd.abs(), dist) and torch.equal(sd < 0, inside & (dist > 0))
        bounded = E.signed_distance(_dev(p), index, bound=0.05)
        near = dist <= 0.05
        assert torch.equal(bounded[near], sd[near]) and bool(torch.isinf(bounded[~near]).all())
        if name == "cube":                                                      # inside a convex body the depth is the distance
            assert np.abs(sd.cpu().numpy() + depth)[depth > 0].max() <= 1e-15
    assert E.contains_points(torch.zeros((0, 3), dtype=torch.float64, device=DEV), index).shape == (0,)


def test_double_walls_show_in_the_count():
    """two parallel sheets a small gap apart, a MeshUDF artefact: the depth buffer sees one face per pixel, the count
    along the normal says 2"""
    from neuraludf_amd import meshrender
    import meshraster_scenes as scenes
    E = _E()
    gap = 2.0 ** -9
    v0, f0 = scenes.sheet(10, lambda u, w: (u, w, 2.0 + 0 * u))
    v = np.concatenate([v0, v0 + np.array([0.0, 0.0, gap])])
    f = np.concatenate([f0, f0[:, ::-1] + len(v0)])                              # the second wall wound the other way
    P = scenes.pinhole(40.0, 32.0, 24.0)[None]
    raster = meshrender.rasterize(_dev(v), _dev(f), _dev(P), 48, 64)
    covered = (raster.face[0] >= 0).cpu().numpy()
    assert covered.sum() > 1000 and (raster.face[0][raster.face[0] >= 0] < len(f0)).all()    # the near wall only
    py, px = np.nonzero(covered)
    d = np.stack([(px - 32.0) / 40.0, (py - 24.0) / 40.0, np.ones(len(px))], -1)             # the pixel-centre rays
    o = np.zeros_like(d)
    index = E.MeshIndex(_dev(v), _dev(f))
    count = index.cast(_dev(o), _dev(d), mode="count").cpu().numpy()
    assert np.array_equal(count, R.cast(o, d, v, f, mode="count"))
    interior = (np.abs(d[:, 0] * 2.0) < 0.99) & (np.abs(d[:, 1] * 2.0) < 0.99)
    assert interior.sum() > 1000 and (count[interior] == 2).all() and count.max() == 2
    first = index.cast(_dev(o), _dev(d))
    assert bool((first.t == 2.0).all())
    beyond = index.cast(_dev(o), _dev(d), t_min=2.0 + gap / 2)
    assert float((beyond.t[torch.from_numpy(interior).to(DEV)] - (2.0 + gap)).abs().max()) <= 1e-14


# ---- 5. against the rasteriser -----------------------------------------------------------------------------------------------
def test_first_hit_agrees_with_the_rasteriser():
    """the pixel-centre rays of the rasteriser's convention (pixel (px, py) is the screen point (px, py); with the
    direction K^-1 (px, py, 1) turned into the world, t is the camera depth itself) on the tilted sheet at 64 x 48: the
    same face wherever both restatements put the pixel more than 1e-9 (in weight) inside its face, and the same depth
    up to the float32 rounding of the raster's output, 2^-24 relative, plus 1e-12 for the float64 evaluations that
    differ (some twenty operations each at 1.1e-16).  The share of pixels left out comes from the two restatements on
    the CPU: the view puts the column px = 32 and the row py = 24 exactly on the sheet's middle edges, 75 of the 1 441
    covered pixels, and the cap is that share."""
    from neuraludf_amd import meshrender
    import meshraster_ref as RR
    import meshraster_scenes as scenes
    E = _E()
    H, W = scenes.VIS_H, scenes.VIS_W
    v, f = scenes.tilted_sheet(30.0)
    P = scenes.VIS_P
    depth_r, face_r, bary_r = RR.rasterize(v, f, P, H, W)
    py, px = np.mgrid[0:H, 0:W]
    d = np.stack([(px.reshape(-1) - 32.0) / 60.0, (py.reshape(-1) - 24.0) / 60.0, np.ones(H * W)], -1)
    o = np.zeros_like(d)
    t_c, face_c, bary_c = R.cast(o, d, v, f)
    covered = (face_r[0].reshape(-1) >= 0) | (face_c >= 0)
    safe = covered & (face_r[0].reshape(-1) >= 0) & (face_c >= 0)
    safe &= (bary_r[0].reshape(-1, 3).min(1) > 1e-9) & (np.nan_to_num(bary_c, nan=0.0).min(1) > 1e-9)
    left_out = covered & ~safe
    print(f"covered {covered.sum()}, left out {left_out.sum()}")
    assert covered.sum() >= 1200 and left_out.sum() <= LEFT_OUT_PIXELS
    raster = meshrender.rasterize(_dev(v), _dev(f), _dev(P), H, W)
    hits = E.cast_rays(_dev(o), _dev(d), _dev(v), _dev(f))
    _same(tuple(hits), (t_c, face_c, bary_c), "pixel-centre rays")
    face_g = raster.face[0].reshape(-1).cpu().numpy().astype(np.int64)
    depth_g = raster.depth[0].reshape(-1).cpu().numpy().astype(np.float64)
    t_g = hits.t.cpu().numpy()
    assert np.array_equal(face_g[safe], face_c[safe])
    assert (np.abs(depth_g[safe] - t_g[safe]) <= (2.0 ** -24 + 1e-12) * t_g[safe]).all()
    assert np.isinf(t_g[~covered]).all() and (face_g[~covered] == -1).all()


LEFT_OUT_PIXELS = 75


# ---- 6. render_image(mesh=...) -------------------------------------------------------------------------------------------------
def test_render_image_with_a_mesh():
    from neuraludf_amd import synth
    from neuraludf_amd.train import Trainer
    E = _E()
    from neuraludf_amd.dataset import RayBatchSource
    scene = synth.make_scene("tiny")
    dummy = torch.zeros(2, scene.H, scene.W, 3)
    source = RayBatchSource(dummy, torch.ones_like(dummy), scene.intrinsics[:2], scene.c2w[:2])
    tr = Trainer(DEV, dict(n_samples=16, n_importance=8, n_outside=0, up_sample_steps=1, perturb=0.0), seed=0)
    v, f = R.icosphere(2, 0.5)
    plain = tr.render_image(source, 0, resolution_level=8)
    with_mesh = tr.render_image(source, 0, resolution_level=8, mesh=(_dev(v), _dev(f)))
    assert set(with_mesh) == set(plain) | {"mesh_depth"}
    for k in plain:
        assert torch.equal(plain[k], with_mesh[k]), k
    md = with_mesh["mesh_depth"]
    assert md.shape == plain["depth"].shape and md.dtype == torch.float64
    rays_o, rays_d = source.gen_rays_at(0, resolution_level=8)
    hits = E.cast_rays(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), _dev(v), _dev(f))
    assert torch.equal(torch.isfinite(md).reshape(-1), hits.face >= 0) and torch.equal(md.reshape(-1), hits.t)
    assert 0 < int(torch.isfinite(md).sum()) < md.numel()
    index = E.MeshIndex(_dev(v), _dev(f))
    assert torch.equal(tr.render_image(source, 0, resolution_level=8, mesh=index)["mesh_depth"], md)
