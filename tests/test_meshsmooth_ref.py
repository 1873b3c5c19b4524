"""CPU: the numpy restatement of the smoothing kernels (tests/meshsmooth_ref.py) against independent expressions -- the
uniform step against D^-1 A applied with scipy.sparse, the cotangent weights against the per-edge (cot alpha + cot beta) / 2
assembly, the vertex-sharing face neighbourhood against sets -- and the behaviour the filters are wanted for, measured on
the restatement: Taubin smoothing without shrinkage, a cube denoised without rounded edges."""
import numpy as np
import pytest

import meshray_ref
import meshsmooth_ref as S


def _meshes():
    cube = S.cube_mesh(8)
    return dict(sphere=meshray_ref.icosphere(2), cube=cube[:2], sheet=S.noisy_sheet()[:2], fan=S.fan_mesh(),
                three=S.three_on_an_edge(), awkward=S.awkward_mesh())


MESHES = _meshes()


def test_test_meshes_have_the_stated_sizes():
    v, f = meshray_ref.icosphere(3)
    assert (len(v), len(f)) == (642, 1280)
    v, f, side = S.cube_mesh(8)
    assert (len(v), len(f)) == (386, 768) and side.shape == (768, 3)
    np.testing.assert_array_equal(S.frames(v, f)[0], side)                  # wound outward, axis-aligned
    v, f, inside = S.noisy_sheet()
    assert (len(v), len(f), int(inside.sum())) == (169, 288, 121)
    assert len(S.fan_mesh()[1]) == 40
    v, f = S.awkward_mesh()
    fn, area, _ = S.frames(v, f)
    assert (fn[-4:] == 0.0).all() and (area[-4:] == 0.0).all() and (area[:-4] > 0).all()
    assert not S.adjacency_sets(f, len(v))[16]                               # the isolated vertex


@pytest.mark.parametrize("name", sorted(MESHES))
def test_uniform_step_is_the_random_walk_matrix(name):
    sp = pytest.importorskip("scipy.sparse")
    v, f = MESHES[name]
    n = len(v)
    rows, cols = [], []
    for t in f:
        for k in range(3):
            if t[k] != t[(k + 1) % 3]:
                rows += [t[k], t[(k + 1) % 3]]
                cols += [t[(k + 1) % 3], t[k]]
    A = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    A.data[:] = 1.0                                                          # duplicates were summed: an edge counts once
    deg = np.asarray(A.sum(1)).reshape(-1)
    mean = A @ v / np.maximum(deg, 1.0)[:, None]
    want = np.where((deg > 0)[:, None], v + 0.37 * (mean - v), v)
    got = S.laplace_step(v, f, 0.37, "uniform")
    np.testing.assert_allclose(got, want, rtol=0, atol=32 * np.finfo(np.float64).eps * np.abs(v).max())
    off, nbr = S.vertex_adjacency(f, n)
    np.testing.assert_array_equal(off[1:] - off[:-1], deg.astype(np.int64))
    np.testing.assert_array_equal(nbr, A.indices)                            # CSR columns are ascending too


@pytest.mark.parametrize("name", ["sphere", "cube"])
def test_cotangent_weights_equal_the_per_edge_assembly(name):
    """on a closed manifold the corner walk adds, for the edge (v, w), max(cot, 0) / 2 of the two angles opposite it"""
    v, f = MESHES[name]
    n = len(v)
    W = np.zeros((n, n))
    for t in f:
        for k in range(3):
            i, j, o = t[k], t[(k + 1) % 3], t[(k + 2) % 3]                   # the angle at o is opposite the edge (i, j)
            a, b = v[i] - v[o], v[j] - v[o]
            cot = a.dot(b) / np.linalg.norm(np.cross(a, b))
            W[i, j] += 0.5 * max(cot, 0.0)
            W[j, i] += 0.5 * max(cot, 0.0)
    mean = W @ v / W.sum(1)[:, None]
    want = v + 0.5 * (mean - v)
    got = S.laplace_step(v, f, 0.5, "cotangent")
    np.testing.assert_allclose(got, want, rtol=0, atol=64 * np.finfo(np.float64).eps)


def test_cotangent_step_keeps_a_regular_sphere_radial():
    v, f = meshray_ref.icosphere(2)
    got = S.laplace_step(v, f, 0.5, "cotangent")
    cosine = (got * v).sum(1) / np.linalg.norm(got, axis=1)
    assert cosine.min() > 1 - 1e-3                                           # the cotangent Laplacian is the mean curvature normal


@pytest.mark.parametrize("name", sorted(MESHES))
def test_face_neighbourhood_equals_the_sets(name):
    v, f = MESHES[name]
    of_vertex = [set() for _ in range(len(v))]
    for i, t in enumerate(f):
        for x in t:
            of_vertex[x].add(i)
    repeats = np.array([len(set(t)) < 3 for t in f.tolist()])                # zero normal whatever the positions: skipped
    for i, row in enumerate(S.face_neighbours(f, len(v))):
        proper = [j for j in row if not repeats[j]]
        assert len(proper) == len(set(proper)), (i, row)                     # every neighbour that can count, once
        assert set(row) == set().union(*(of_vertex[x] for x in f[i])) - {i}, i


def test_visiting_order_does_not_depend_on_the_winding():
    v, f = S.noisy_cube()[:2]
    rng = np.random.default_rng(3)
    g = f.copy()
    flip = rng.random(len(f)) < 0.5
    g[flip] = g[flip][:, [0, 2, 1]]
    assert S.face_neighbours(f, len(v)) == S.face_neighbours(g, len(v))
    pa, na = S.denoise_mesh(v, f)
    pb, nb = S.denoise_mesh(v, g)
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(np.where(flip[:, None], -nb, nb), na)


def test_degenerate_and_fixed_vertices_stay():
    v, f = S.awkward_mesh()
    for w in ("uniform", "cotangent"):
        out = S.smooth_mesh(v, f, 3, weights=w, boundary="free")
        np.testing.assert_array_equal(out[16], v[16])                        # isolated
        assert np.abs(out - v).max() > 1e-3
    out = S.smooth_mesh(v, f, 3, weights="cotangent", boundary="free")
    np.testing.assert_array_equal(out[17], v[17])                            # its faces repeat a vertex: degenerate for good
    out = S.smooth_mesh(v, f, 1, mu=0.0, weights="cotangent", boundary="free")
    np.testing.assert_array_equal(out[17:], v[17:])                          # 18: its one face has no area in this step
    out, fn = S.denoise_mesh(v, f, boundary="free")
    np.testing.assert_array_equal(out[16:], v[16:])
    assert (fn[-4:] == 0.0).all() and np.isfinite(out).all()
    mask = np.zeros(len(v), bool)
    mask[[5, 6]] = True
    out = S.smooth_mesh(v, f, 3, boundary="free", fixed=mask)
    np.testing.assert_array_equal(out[mask], v[mask])
    v, f, inside = S.noisy_sheet()
    np.testing.assert_array_equal(S.smooth_mesh(v, f)[~inside], v[~inside])
    assert np.abs(S.smooth_mesh(v, f, boundary="free")[~inside] - v[~inside]).max() > 1e-3
    assert S.smooth_mesh(v, f, 0) is v and S.smooth_mesh(v.astype(np.float32), f).dtype == np.float32


def test_taubin_does_not_shrink_the_sphere():
    """the caps of the GPU test, on the restatement: measured 0.00997 -> 0.0049 / 0.00286, radii 1.0029 / 0.945 / 0.99985"""
    v, f = S.noisy_sphere()
    rms0, _ = S.radial_stats(v)
    rms, radius = S.radial_stats(S.smooth_mesh(v, f, 10, 0.5, -0.53))
    assert rms < 0.6 * rms0 and abs(radius - 1.0) < 0.005, (rms0, rms, radius)
    assert S.radial_stats(S.smooth_mesh(v, f, 10, 0.5, 0.0))[1] < 0.96
    rms, radius = S.radial_stats(S.denoise_mesh(v, f)[0])
    assert rms < 0.4 * rms0 and abs(radius - 1.0) < 0.001, (rms0, rms, radius)


def test_denoising_keeps_the_cube_edges():
    """measured: 8.2 degrees -> 0.96 after denoise_mesh, 10.6 after Taubin smoothing"""
    v, f, side = S.noisy_cube()
    before = S.mean_normal_angle(S.frames(v, f)[0], side)
    out, fn = S.denoise_mesh(v, f)
    after = S.mean_normal_angle(S.frames(out, f)[0], side)
    assert after < 2.0 and after < before / 3.0, (before, after)
    np.testing.assert_allclose(np.linalg.norm(fn, axis=1), 1.0, atol=1e-14)
    assert S.mean_normal_angle(S.frames(S.smooth_mesh(v, f), f)[0], side) > before


@pytest.mark.parametrize("weights", ["uniform", "cotangent"])
def test_sheet_noise_is_halved(weights):
    """measured: interior RMS height 0.0092 -> 0.0041 (uniform), 0.0043 (cotangent)"""
    v, f, inside = S.noisy_sheet()
    out = S.smooth_mesh(v, f, weights=weights)
    rms = lambda x: float(np.sqrt(np.mean(x[inside, 2] ** 2)))
    assert rms(out) < 0.5 * rms(v), (rms(v), rms(out))
