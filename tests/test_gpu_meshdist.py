"""GPU: exact point-to-mesh distance (neuraludf_amd/evaluation.py MeshIndex / closest_on_mesh / mesh_deviation,
csrc/meshdist.hip) against the numpy restatement (tests/meshdist_ref.py) bit for bit, and what it enables in
neuraludf_amd/meshclean.py: simplify_to_error, transfer_attributes, simplify_mesh(measure=True), the two CLIs.  What it
replaces: trimesh.proximity.closest_point on the CPU, or a KD-tree over surface samples."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshdist_ref as R
import meshsimplify_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _np(c):
    return tuple(t.cpu().numpy() for t in c)


def _same(got, want, what=""):
    for name, g, w in zip(("dist", "face", "point", "bary"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            rows = np.unique(np.argwhere(g.view(np.int64) != w.view(np.int64))[:, 0])[:5]
            raise AssertionError((what, name, rows.tolist(), g[rows].tolist(), w[rows].tolist()))


def _closest(q, v, f, **kw):
    return _np(_E().closest_on_mesh(_dev(q), _dev(v), _dev(f), **kw))


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

    add(*S.sphere_mesh(24))                                                            # closed, marching cubes
    sv, sf = S.sheet(8, -0.9, -0.3)
    add(sv + np.array([0.0, 0.0, 0.8]), sf)                                            # an open sheet
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


def _mixed_queries(v, f, rng):
    ok = R.usable_faces(v, f)
    fu = f[ok]
    verts = v[np.unique(fu)]
    e = fu[rng.integers(0, len(fu), 600)]
    mids = 0.5 * (v[e[:, 0]] + v[e[:, 1]])
    t = fu[rng.integers(0, len(fu), 600)]
    w = rng.dirichlet((1.0, 1.0, 1.0), 600)
    near = (w[:, :, None] * v[t]).sum(1) + rng.normal(scale=1e-9, size=(600, 3))
    box = rng.uniform(-1.1, 1.1, (1500, 3))
    diag = float(np.linalg.norm(np.nanmax(v, 0) - np.nanmin(v, 0)))
    d = rng.normal(size=(6, 3))
    far = 100.0 * diag * d / np.linalg.norm(d, axis=1, keepdims=True)
    q = np.concatenate([verts, mids, near, box, far])
    dup = q[rng.integers(0, len(q), 4000 - len(q))] if len(q) < 4000 else q[:0]
    q = np.concatenate([q, dup])
    return q[rng.permutation(len(q))]


@pytest.fixture(scope="module")
def mixed():
    """the mixed mesh, its queries and the restatement's answer, computed once and left unchanged"""
    rng = np.random.default_rng(21)
    v, f = _mixed_mesh()
    q = _mixed_queries(v, f, rng)
    want = R.closest(q, v, f)
    for a in (v, f, q) + want:
        a.setflags(write=False)
    return v, f, q, want


def test_mixed_mesh_at_three_cell_sizes(mixed):
    v, f, q, want = mixed
    E = _E()
    assert 1500 <= len(f) <= 3000 and len(q) >= 4000
    index = E.MeshIndex(_dev(v), _dev(f))
    ext = float(np.nanmax(v) - np.nanmin(v))
    got = _np(index.closest(_dev(q)))
    _same(got, want, "default cell")
    assert (got[0] == 0).sum() >= 500 and np.isfinite(got[0]).all()
    for cell in (index.cell / 4, 4.0 * ext):
        other = E.MeshIndex(_dev(v), _dev(f), cell=cell)
        assert other.cell == cell and other.n_refs != index.n_refs
        _same(_np(E.closest_on_mesh(_dev(q), index=other)), want, f"cell {cell}")
    assert E.MeshIndex(_dev(v), _dev(f), cell=4.0 * ext).n_cells == 1
    # the NaN face is absent, the duplicated faces lose to their originals, float32 queries are widened exactly
    assert len(f) - 3 not in got[1] and (got[1] < len(f) - 2).all()
    _same(_np(E.closest_on_mesh(_dev(q.astype(np.float32)), index=index)),
          R.closest(q.astype(np.float32).astype(np.float64), v, f), "float32 queries")


# ---- 2. one large face among small ones ------------------------------------------------------------------------------------
def test_one_large_face_among_small_ones():
    rng = np.random.default_rng(22)
    big = np.array([[0.0, 0.0, 0.0], [21.0, 2.0, 21.0], [2.0, 21.0, 21.0]])
    pv, pf = S.sheet(10, 5.0, 15.0)                                            # 200 faces of cell size below its box
    v = np.concatenate([big, pv + np.array([0.0, 0.0, -3.0])])
    f = np.concatenate([[[0, 1, 2]], pf + 3])
    q = np.concatenate([rng.uniform(-8.0, 25.0, (1200, 3)),
                        np.stack([rng.uniform(4, 16, 300), rng.uniform(4, 16, 300), rng.uniform(-6, 1, 300)], -1),
                        np.array([[-6.0, -6.0, -6.0], [-7.5, 1.0, -5.0], [25.0, 25.0, 30.0]])])
    E = _E()
    index = E.MeshIndex(_dev(v), _dev(f), cell=1.0)
    assert index.cell == 1.0 and index.n_refs >= 21 ** 3 + 200
    want = R.closest(q, v, f)
    got = _np(index.closest(_dev(q)))
    _same(got, want, "large face")
    large = got[1] == 0
    outside = (q < -3.0).any(1)                                                # three cells and more outside its box
    assert (large & outside).sum() >= 20 and (~large).sum() >= 100 and (large & ~outside).sum() >= 100
    _same(_closest(q, v, f), want, "large face, default cell")


# ---- 3. bound ------------------------------------------------------------------------------------------------------------
def test_bound(mixed):
    v, f, q, want = mixed
    bound = float(np.percentile(want[0], 60))               # above the queries that lie on the mesh, among the box's
    assert np.percentile(want[0], 30) < bound < np.percentile(want[0], 70)
    got = _closest(q, v, f, bound=bound)
    beyond = want[0] > bound
    assert 0.3 * len(q) <= beyond.sum() <= 0.7 * len(q)
    masked = [np.array(a) for a in want]
    masked[0][beyond], masked[1][beyond], masked[2][beyond], masked[3][beyond] = np.inf, -1, np.nan, np.nan
    _same(got, masked, "bound")
    lo, hi = np.nanmin(v[np.unique(f[R.usable_faces(v, f)])], 0), np.nanmax(v[np.unique(f[R.usable_faces(v, f)])], 0)
    box_d = np.linalg.norm(np.maximum(np.maximum(lo - q, q - hi), 0.0), axis=1)
    assert (box_d > bound * 1.001).sum() >= 6 and beyond[box_d > bound * 1.001].all()          # the early exit's rows
    # a bound that is a distance itself keeps that row (<=)
    k = int(np.argsort(want[0])[len(q) // 2])
    assert _closest(q[k:k + 1], v, f, bound=float(want[0][k]))[1][0] == want[1][k]


# ---- 4. key width --------------------------------------------------------------------------------------------------------
def test_keys_beyond_2_to_the_59():
    rng = np.random.default_rng(24)
    step = float(1 << 20)
    base = rng.uniform(0.0, 3.0, (100, 1, 3)) + rng.uniform(-0.15, 0.15, (100, 3, 3))
    v = np.concatenate([base.reshape(-1, 3), base.reshape(-1, 3) + step])
    f = np.arange(600, dtype=np.int64).reshape(200, 3)
    q = np.concatenate([rng.uniform(-2.0, 5.0, (100, 3)), rng.uniform(-2.0, 5.0, (100, 3)) + step])
    E = _E()
    index = E.MeshIndex(_dev(v), _dev(f), cell=1.0)
    assert index.cell == 1.0 and min(index.grid) > 1 << 20
    assert int(index.cell_key.max()) > 1 << 59
    want = R.closest(q, v, f, bound=1.5)
    got = _np(index.closest(_dev(q), bound=1.5))
    _same(got, want, "key width")
    assert (got[1][:100] >= 0).sum() > 20 and (got[1][100:] >= 100).sum() > 20 and (got[1] == -1).sum() > 5
    assert not (got[1][:100] >= 100).any() and not ((got[1][100:] >= 0) & (got[1][100:] < 100)).any()


# ---- 5. the edges of the domain ------------------------------------------------------------------------------------------
def test_edges_of_the_domain():
    E = _E()
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [3.0, 3.0, 3.0], [2.0, 0.0, 0.0]])
    f = np.array([[0, 1, 2]])
    empty = E.closest_on_mesh(torch.zeros((0, 3), dtype=torch.float64, device=DEV), _dev(v), _dev(f))
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 3), (0, 3)] and empty.face.dtype == torch.int64
    q = np.array([[0.25, 0.25, 2.0], [-3.0, -4.0, 0.0], [0.5, -2.0, 0.0], [1.0, 1.0, 0.0]])
    got = _closest(q, v, f)                                                    # a single face
    _same(got, R.closest(q, v, f), "single face")
    assert got[0].tolist() == [2.0, 5.0, 2.0, math.sqrt(0.5)]
    degenerate = np.array([[0, 1, 4], [3, 3, 3], [1, 1, 0]])                   # a segment, a point, a segment
    got = _closest(q, v, degenerate)
    _same(got, R.closest(q, v, degenerate), "degenerate faces")
    assert got[0][0] == math.sqrt(0.0625 + 4.0) and got[0][1] == 5.0
    again = _closest(q, v, degenerate)
    _same(again, got, "second run")
    with pytest.raises(ValueError, match="no faces"):
        E.MeshIndex(_dev(v), torch.zeros((0, 3), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="out of range"):
        E.MeshIndex(_dev(v), _dev(np.array([[0, 1, 5]])))
    with pytest.raises(ValueError, match="out of range"):
        E.MeshIndex(_dev(v), _dev(np.array([[0, -1, 2]])))
    with pytest.raises(ValueError, match="infinite"):
        E.MeshIndex(_dev(np.where(v == 3.0, np.inf, v)), _dev(f))
    with pytest.raises(ValueError, match="usable"):
        E.MeshIndex(_dev(np.where(v == 1.0, np.nan, v)), _dev(f))
    with pytest.raises(ValueError, match="max_refs"):
        E.MeshIndex(_dev(v), _dev(degenerate), max_refs=2)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            E.closest_on_mesh(_dev(np.array([[0.0, bad, 0.0]])), _dev(v), _dev(f))
    with pytest.raises(ValueError, match="bound"):
        E.closest_on_mesh(_dev(q), _dev(v), _dev(f), bound=0.0)
    with pytest.raises(ValueError):
        E.closest_on_mesh(_dev(q), _dev(v), _dev(f), index=E.MeshIndex(_dev(v), _dev(f)))
    # max_refs makes the cell grow until the references fit
    sv, sf = S.sheet(16, 0.0, 1.0)
    fine = E.MeshIndex(_dev(sv), _dev(sf), cell=1.0 / 64)
    coarse = E.MeshIndex(_dev(sv), _dev(sf), cell=1.0 / 64, max_refs=fine.n_refs // 2)
    assert coarse.cell > fine.cell and len(sf) <= coarse.n_refs <= fine.n_refs // 2


# ---- 6. mesh_deviation ---------------------------------------------------------------------------------------------------
def _pow2_sheet(lift=0.0):
    v, f = S.sheet(16, 0.0, 1.0)                                               # spacing 2^-4: every normal a power of two
    return v + np.array([0.0, 0.0, lift]), f


def test_mesh_deviation():
    E = _E()
    v, f = _pow2_sheet()
    same = E.mesh_deviation((_dev(v), _dev(f)), (_dev(v), _dev(f)))
    zero = dict(max=0.0, mean=0.0, rms=0.0, n=len(v))
    assert same == dict(a_to_b=zero, b_to_a=zero, hausdorff=0.0)
    up, _ = _pow2_sheet(2.0 ** -7)
    dev = E.mesh_deviation((_dev(v), _dev(f)), (_dev(up), _dev(f)))
    one = dict(max=2.0 ** -7, mean=2.0 ** -7, rms=2.0 ** -7, n=len(v))
    assert dev == dict(a_to_b=one, b_to_a=one, hausdorff=2.0 ** -7)
    index = E.MeshIndex(_dev(up), _dev(f))                                     # an index stands for its mesh
    assert E.mesh_deviation((_dev(v), _dev(f)), index) == dev
    dense = E.mesh_deviation((_dev(v), _dev(f)), (_dev(up), _dev(f)), density=0.02)
    n = E.sample_mesh(_dev(v), _dev(f), 0.02).shape[0]
    assert dense["a_to_b"]["n"] == dense["b_to_a"]["n"] == n > 4 * len(v)
    assert dense["hausdorff"] == 2.0 ** -7 and abs(dense["a_to_b"]["mean"] - 2.0 ** -7) <= 1e-15
    far = E.mesh_deviation((_dev(v), _dev(f)), (_dev(up), _dev(f)), bound=2.0 ** -8)
    assert far["hausdorff"] == math.inf
    text = E.format_deviation(dev)
    assert text == ("a_to_b max 0.007812 mean 0.007812 rms 0.007812 n 289 \n"
                    "b_to_a max 0.007812 mean 0.007812 rms 0.007812 n 289 \nhausdorff 0.007812 \n")


# ---- 7. simplify_to_error ------------------------------------------------------------------------------------------------
def test_simplify_to_error():
    from neuraludf_amd import meshing
    E = _E()
    v, f = S.folded_sheet()
    assert len(f) == 4608
    dv, df = _dev(v), _dev(f)
    max_error = 0.08                                          # the sheet's quads measure 0.034
    s, dev = meshing.simplify_to_error(dv, df, max_error)
    assert isinstance(s, meshing.Simplified)
    assert 0 < dev["hausdorff"] <= max_error and 0 < s.faces.shape[0] < len(f)
    assert dev == E.mesh_deviation((dv, df), (s.verts, s.faces))
    assert dev["a_to_b"]["n"] == len(v) and dev["b_to_a"]["n"] == s.verts.shape[0]
    print(f"simplify_to_error {max_error}: {s.faces.shape[0]} faces, hausdorff {dev['hausdorff']:.4g}")
    tight = meshing.simplify_to_error(dv, df, max_error / 4)[0]
    assert s.faces.shape[0] < tight.faces.shape[0] < len(f)
    # the same figures from simplify_mesh(measure=True), and nothing changes without it
    info = {}
    cell = 0.1
    plain = meshing.simplify_mesh(dv, df, cell)
    measured, mdev = meshing.simplify_mesh(dv, df, cell, measure=True, _info=info)
    assert all(torch.equal(a, b) for a, b in zip(plain[:5], measured[:5]))
    assert info["deviation"] == mdev == E.mesh_deviation((dv, df), (plain.verts, plain.faces))
    assert 0 < mdev["hausdorff"] <= math.sqrt(3.0) * cell
    # a bound nothing meets: the input comes back
    same, zero = meshing.simplify_to_error(dv, df, 1e-30)
    assert same.verts is dv or torch.equal(same.verts, dv)
    assert torch.equal(same.faces, df) and bool(same.accepted.all()) and same.accepted.shape[0] == len(v)
    assert torch.equal(same.vertex_cluster, torch.arange(len(v), device=DEV))
    assert torch.equal(same.face_src, torch.arange(len(f), device=DEV))
    assert zero["hausdorff"] == 0.0 and zero["a_to_b"]["max"] == zero["b_to_a"]["rms"] == 0.0
    with pytest.raises(ValueError):
        meshing.simplify_to_error(dv, df, -1.0)
    with pytest.raises(ValueError):
        meshing.simplify_to_error(dv, df, 0.1, cell=0.1)


# ---- 8. transfer_attributes ----------------------------------------------------------------------------------------------
def test_transfer_attributes():
    from neuraludf_amd import meshing
    E = _E()
    G = np.array([[0.3, -0.2, 0.5], [0.1, 0.4, -0.3], [-0.6, 0.2, 0.1]])
    c0 = np.array([0.5, 0.4, 0.3])
    for v, f in (S.sheet(), S.folded_sheet()):
        dv, df = _dev(v), _dev(f)
        colours = _dev(v @ G + c0)
        s = meshing.simplify_mesh(dv, df, 0.11)
        got = meshing.transfer_attributes(dv, df, colours, s.verts)
        assert got.shape == (s.verts.shape[0], 3) and got.dtype == torch.float64
        c = E.closest_on_mesh(s.verts, dv, df)
        there = c.point.cpu().numpy() @ G + c0                                 # the linear function at the closest point
        assert np.abs(got.cpu().numpy() - there).max() <= 1e-9
        on = (c.dist <= 1e-12).cpu().numpy()                                   # destinations on the source surface
        if v[:, 2].max() == 0.0:
            assert on.sum() >= 0.5 * len(on)
        assert np.abs(got.cpu().numpy() - (s.verts.cpu().numpy() @ G + c0))[on].max(initial=0.0) <= 1e-9
    dst = torch.cat([s.verts[:10], s.verts[:5] + 7.0])
    bounded = meshing.transfer_attributes(dv, df, colours.float(), dst, bound=1.0)
    assert bounded.dtype == torch.float32 and bool(torch.isnan(bounded[10:]).all())
    assert float((bounded[:10].double() - got[:10]).abs().max()) <= 1e-6          # float32 in, float32 out
    with pytest.raises(ValueError):
        meshing.transfer_attributes(dv, df, colours[:-1], dst)


# ---- 9. the CLIs ---------------------------------------------------------------------------------------------------------
def test_cli_deviation(tmp_path):
    from neuraludf_amd import meshing
    E = _E()
    v, f = _pow2_sheet()
    up, _ = _pow2_sheet(2.0 ** -7)
    meshing.write_ply(tmp_path / "a.ply", v, f)
    meshing.write_ply(tmp_path / "b.ply", up, f)
    log = tmp_path / "dev.txt"
    p = subprocess.run([sys.executable, "-m", "neuraludf_amd.evaluation", "deviation", "--a", str(tmp_path / "a.ply"),
                        "--b", str(tmp_path / "b.ply"), "--log", str(log)],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    one = dict(max=2.0 ** -7, mean=2.0 ** -7, rms=2.0 ** -7, n=len(v))
    assert log.read_text() == E.format_deviation(dict(a_to_b=one, b_to_a=one, hausdorff=2.0 ** -7))
    assert "hausdorff: 0.0078125" in p.stdout and "a_to_b: max: 0.0078125; mean: 0.0078125; rms: 0.0078125; n: 289." in p.stdout


def test_cli_simplify_max_error(tmp_path):
    from neuraludf_amd import meshing
    E = _E()
    v, f = S.folded_sheet()
    v = v.astype(np.float32)
    meshing.write_ply(tmp_path / "in.ply", v, f)
    p = subprocess.run([sys.executable, "-m", "neuraludf_amd.meshing", str(tmp_path / "in.ply"), str(tmp_path / "out.ply"),
                        "--simplify-max-error", "0.02"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("simplify: deviation hausdorff ")]
    assert len(line) == 1
    printed = float(line[0].split()[3])
    assert 0 < printed <= 0.02
    ov, of = meshing.read_ply(tmp_path / "out.ply")
    assert 0 < len(of) < len(f)
    again = E.mesh_deviation((_dev(v.astype(np.float64)), _dev(f)), (_dev(ov), _dev(of)))     # the file is float32
    assert abs(again["hausdorff"] - printed) <= 1e-6
    p = subprocess.run([sys.executable, "-m", "neuraludf_amd.meshing", str(tmp_path / "in.ply"), str(tmp_path / "x.ply"),
                        "--simplify-max-error", "0.02", "--simplify-to", "100"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), timeout=300)
    assert p.returncode != 0 and "not allowed with" in p.stderr
