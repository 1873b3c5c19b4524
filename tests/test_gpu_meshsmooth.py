"""GPU: mesh smoothing and denoising (neuraludf_amd/meshclean.py smooth_mesh / denoise_mesh / vertex_adjacency,
csrc/meshsmooth.hip) against the numpy restatement (tests/meshsmooth_ref.py): the Laplacian steps, the face frames, the
vertex update and the adjacency bit for bit, the bilateral normal step and denoise_mesh to the bounds worked out below --
plus what the filters are for (a sphere that does not shrink, a cube that keeps its edges), the mesher end to end and the
CLI.  What it adds to the reference: extract_mesh.py:238-265 smooths border vertices only.

The bound of one normal step.  Kernel and restatement are fed the same bits and apply the same operations, except for the
exp of the weight: ROCm documents 1 ulp for the float64 exp of its device library, the GNU C library 1 ulp for its own, so
with u = 2^-52 the two weights differ by at most 2 u relative, 3 u after the product with the area and 4 u |w| in each
term w n'.  The end-to-end run adds 12 u for sigma_c, whose mean either side may round differently (4 u on 1 / (2 sigma_c^2),
times a spatial exponent that the test meshes keep below 3).  A face has K neighbours; each of the K additions rounds on
either side, u / 2 of a partial sum that is at most W = the sum of the weights.  So each component of s differs by at most
(16 + K) u W, s by sqrt(3) times that, and the unit vector by twice that over |s| plus 3 u for the square root and the
division: T = (2 sqrt(3) (K + 16) / rho + 3) u with rho = |s| / W.  K and rho are read from the restatement, never from
the kernel; the test asserts K <= 64 and rho >= 0.25, where T = 2.5e-13.

Steps in sequence.  An error e in every normal moves a weight by at most 4 sqrt(2) e / (2 sigma_s^2) relative (|n_i - n_j'|
<= sqrt(2) after the turn into n_i's half-space) and the term by e more, so the next step starts from
L e + T with L = 2 (1 + 4 sqrt(2) / (2 sigma_s^2)) / rho: about 50 at sigma_s = 0.35, rho = 1.  After five steps that bound
is beyond any use, so the steps are checked one by one, each fed the restatement's previous normals (bound T), and
denoise_mesh end to end at two normal steps, e = (L + 1) T, and three vertex steps: one adds 2 e h (|c_f - p| <= h, the
longest edge) and multiplies what the positions carry by at most 7 / 3 (a centre moves by a third of three vertices, the
vertex itself by all of it), so the positions differ by at most 2 e h (1 + 7 / 3 + 49 / 9) + 64 u max |p|.  The test
asserts that this stays below 1e-9 and prints what it measures; the run with the default counts is printed as well and
held to the same 1e-9, which the linear bound cannot promise: it is a measurement against a cap."""
import numpy as np
import pytest
import torch

import meshsmooth_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
U = 2.0 ** -52
K_MAX, RHO_MIN, CAP = 64, 0.25, 1e-9
SIGMA_S = 0.35


def step_bound(k, rho):
    return (2.0 * np.sqrt(3.0) * (k + 16) / rho + 3.0) * U


def chain_factor(rho, sigma_s=SIGMA_S):
    return 2.0 * (1.0 + 4.0 * np.sqrt(2.0) / (2.0 * sigma_s * sigma_s)) / rho


@pytest.fixture(scope="module", autouse=True)
def _hand_back_the_cache():
    """these tests leave float64 geometry in the blocks torch's allocator keeps; buffers that later tests take from it
    with torch.empty would start with those bits in their pad rows.  Hand the blocks back."""
    yield
    torch.cuda.empty_cache()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _build_meshes():
    out = dict(sphere=S.noisy_sphere(), cube=S.noisy_cube()[:2], sheet=S.noisy_sheet()[:2], fan=S.fan_mesh(),
               three=S.three_on_an_edge(), awkward=S.awkward_mesh())
    return {k: _frozen(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)) for k, (v, f) in out.items()}


MESHES = _build_meshes()
NAMES = sorted(MESHES)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # a copy: the fixtures' arrays are read-only


def _mask(name):
    """a random user mask, the same for the kernel and the restatement"""
    rng = np.random.default_rng(len(name))
    return rng.random(len(MESHES[name][0])) < 0.3


@pytest.fixture(scope="module")
def denoised():
    """the restatement's denoise_mesh at the default settings and its statistics, once per mesh"""
    out = {}
    for name, (v, f) in MESHES.items():
        stats = {}
        pos, fn = S.denoise_mesh(v, f, stats=stats)
        out[name] = _frozen(pos, fn) + (stats,)
    return out


class _Kernels:
    """the four entry points on a mesh, through the descriptor, as smooth_mesh and denoise_mesh drive them"""

    def __init__(self, v, f):
        from neuraludf_amd import _lib, meshclean
        self.lib, self.n_faces = _lib, len(f)
        self.pos, self.faces = _dev(v), _dev(f)
        self.corner_off, self.corner = meshclean._corner_lists(self.faces, len(v))
        self.d = _lib.MeshOrient(faces=_lib.ptr(self.faces), pos=_lib.ptr(self.pos), corner_off=_lib.ptr(self.corner_off),
                                 corner=_lib.ptr(self.corner), n_faces=len(f), n_verts=len(v))

    def frames(self):
        from neuraludf_amd import meshclean
        self.fnormal, self.area, self.centre = meshclean._face_frames(self.d, self.n_faces, DEV)
        return [t.cpu().numpy() for t in (self.fnormal, self.area, self.centre)]

    def normals(self, fnormal, sigma_c, sigma_s=SIGMA_S):
        src, out = _dev(fnormal), torch.empty((self.n_faces, 3), dtype=torch.float64, device=DEV)
        self.d.sm_fnormal, self.d.sm_fnormal_out = self.lib.ptr(src), self.lib.ptr(out)
        self.d.sm_inv2sc, self.d.sm_inv2ss = 1.0 / (2.0 * sigma_c * sigma_c), 1.0 / (2.0 * sigma_s * sigma_s)
        self.lib.call("nudf_meshsmooth_normals", self.d)
        return out.cpu().numpy()

    def update(self, pos, fnormal, fixed=None):
        src, fn, out = _dev(pos), _dev(fnormal), torch.empty((len(pos), 3), dtype=torch.float64, device=DEV)
        mask = None if fixed is None else _dev(fixed.astype(np.uint8))
        self.d.pos, self.d.sm_pos_out, self.d.sm_fnormal = self.lib.ptr(src), self.lib.ptr(out), self.lib.ptr(fn)
        self.d.sm_fixed = self.lib.ptr(mask)
        self.lib.call("nudf_meshsmooth_update", self.d)
        self.d.pos = self.lib.ptr(self.pos)
        return out.cpu().numpy()


# ---- bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_vertex_adjacency_equals_the_sets(name):
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    off, nbr = meshing.vertex_adjacency(_dev(f), len(v))
    want_off, want_nbr = S.vertex_adjacency(f, len(v))
    assert off.dtype == nbr.dtype == torch.int64
    np.testing.assert_array_equal(off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(nbr.cpu().numpy(), want_nbr)
    table = meshing.mesh_edges(_dev(f), len(v))
    again = meshing.vertex_adjacency(_dev(f), len(v), table)
    assert torch.equal(again[0], off) and torch.equal(again[1], nbr)
    ring = S.adjacency_sets(f, len(v))
    got = nbr.cpu().numpy()
    assert all(set(got[want_off[i]:want_off[i + 1]]) == ring[i] for i in range(len(v)))


@pytest.mark.parametrize("weights", ["uniform", "cotangent"])
@pytest.mark.parametrize("name", NAMES)
def test_laplace_equals_the_restatement(name, weights):
    """one step, and the driver at 1, 2 and 10 rounds: borders fixed and free, with and without a user mask"""
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    vt, ft = _dev(v), _dev(f)
    for step in (0.5, -0.53):
        got = meshing.smooth_mesh(vt, ft, 1, lam=step, mu=0.0, weights=weights, boundary="free")
        np.testing.assert_array_equal(got.cpu().numpy(), S.laplace_step(v, f, step, weights), err_msg=f"step {step}")
    moved = 0.0
    for iterations in (1, 2, 10):
        for boundary in ("fixed", "free"):
            for mask in (None, _mask(name)):
                got = meshing.smooth_mesh(vt, ft, iterations, weights=weights, boundary=boundary, fixed=_dev(mask))
                want = S.smooth_mesh(v, f, iterations, weights=weights, boundary=boundary, fixed=mask)
                assert got.dtype == torch.float64
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{iterations} {boundary}")
                moved = max(moved, float(np.abs(want - v).max()))
    assert moved > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_frames_equal_the_restatement(name):
    v, f = MESHES[name]
    for got, want, what in zip(_Kernels(v, f).frames(), S.frames(v, f), ("normals", "areas", "centres")):
        np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.mark.parametrize("name", NAMES)
def test_update_equals_the_restatement(name, denoised):
    """one step from the input and one from the restatement's result, fed the restatement's filtered normals"""
    v, f = MESHES[name]
    k = _Kernels(v, f)
    fn = denoised[name][1]
    border = S.border_vertices(f, len(v))
    for pos in (v, denoised[name][0]):
        for fixed in (None, border, _mask(name)):
            np.testing.assert_array_equal(k.update(pos, fn, fixed), S.update_step(pos, f, fn, fixed))
    assert np.abs(S.update_step(v, f, fn) - v).max() > 1e-4


# ---- to the derived bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_normal_steps_one_by_one(name):
    """each of five steps from the restatement's previous normals: within T of the restatement's next"""
    v, f = MESHES[name]
    k = _Kernels(v, f)
    fn, area, centre = S.frames(v, f)
    sigma_c = S.mean_edge_length(v, f)
    inv2sc, inv2ss = 1.0 / (2.0 * sigma_c * sigma_c), 1.0 / (2.0 * SIGMA_S * SIGMA_S)
    nb = S.face_neighbours(f, len(v))
    k.frames()
    worst = 0.0
    for step in range(5):
        stats = {}
        want = S.normals_step(fn, area, centre, inv2sc, inv2ss, nb, stats)
        got = k.normals(fn, sigma_c)
        assert stats["k"] <= K_MAX and stats.get("rho", 1.0) >= RHO_MIN, stats
        bound = step_bound(stats["k"], stats.get("rho", 1.0))
        err = float(np.abs(got - want).max())
        worst = max(worst, err / bound)
        assert err <= bound <= CAP, (step, err, bound)
        zero = (fn == 0.0).all(1)
        np.testing.assert_array_equal(got[zero], 0.0)
        np.testing.assert_allclose(np.linalg.norm(got[~zero], axis=1), 1.0, atol=8 * U)
        fn = want
    print(f"{name}: largest difference of a step {worst:.3g} of its bound {bound:.3g}")


@pytest.mark.parametrize("name", NAMES)
def test_denoise_mesh_within_the_bound(name, denoised):
    from neuraludf_amd import meshing
    v, f = MESHES[name]
    stats = {}
    want_pos, want_fn = S.denoise_mesh(v, f, 2, 3, stats=stats)
    got_pos, got_fn = meshing.denoise_mesh(_dev(v), _dev(f), 2, 3)
    assert got_pos.dtype == got_fn.dtype == torch.float64 and got_fn.shape == (len(f), 3)
    assert stats["k"] <= K_MAX and stats.get("rho", 1.0) >= RHO_MIN, stats
    rho = stats.get("rho", 1.0)
    e = (chain_factor(rho) + 1.0) * step_bound(stats["k"], rho)
    e_fn = float(np.abs(got_fn.cpu().numpy() - want_fn).max())
    edges = S.unique_edges(f, len(v))
    h = float(np.linalg.norm(v[edges[:, 0]] - v[edges[:, 1]], axis=1).max())
    bound = 2.0 * e * h * (1.0 + 7.0 / 3.0 + 49.0 / 9.0) + 64 * U * float(np.abs(v).max())
    e_pos = float(np.abs(got_pos.cpu().numpy() - want_pos).max())
    print(f"{name} (2, 3): normals {e_fn:.3g} (bound {e:.3g}), positions {e_pos:.3g} (bound {bound:.3g})")
    assert e_fn <= e <= CAP and e_pos <= bound <= CAP
    got_pos, got_fn = meshing.denoise_mesh(_dev(v), _dev(f))
    e_fn = float(np.abs(got_fn.cpu().numpy() - denoised[name][1]).max())
    e_pos = float(np.abs(got_pos.cpu().numpy() - denoised[name][0]).max())
    print(f"{name} (defaults): normals {e_fn:.3g}, positions {e_pos:.3g}")
    assert e_fn <= CAP and e_pos <= CAP


# ---- properties, on the GPU results ---------------------------------------------------------------------------------------
def test_what_must_not_move_does_not():
    from neuraludf_amd import meshing
    v, f = MESHES["awkward"]
    vt, ft = _dev(v), _dev(f)
    for w in ("uniform", "cotangent"):
        out = meshing.smooth_mesh(vt, ft, 3, weights=w, boundary="free")
        assert torch.equal(out[16], vt[16])                                   # isolated
        assert float((out - vt).abs().max()) > 1e-3
    out = meshing.smooth_mesh(vt, ft, 3, weights="cotangent", boundary="free")
    assert torch.equal(out[17], vt[17])                                       # its faces repeat a vertex
    out = meshing.smooth_mesh(vt, ft, 1, mu=0.0, weights="cotangent", boundary="free")
    assert torch.equal(out[17:], vt[17:])                                     # 18: its one face has no area in this step
    out, fn = meshing.denoise_mesh(vt, ft, boundary="free")
    assert torch.equal(out[16:], vt[16:]) and bool((fn[-4:] == 0).all()) and bool(torch.isfinite(out).all())
    mask = _mask("awkward")
    for w in ("uniform", "cotangent"):
        out = meshing.smooth_mesh(vt, ft, 3, weights=w, boundary="free", fixed=_dev(mask))
        assert torch.equal(out[_dev(mask)], vt[_dev(mask)])
    assert torch.equal(meshing.denoise_mesh(vt, ft, boundary="free", fixed=mask.tolist())[0][_dev(mask)], vt[_dev(mask)])
    v, f, inside = S.noisy_sheet()
    vt, ft, border = _dev(v), _dev(f), _dev(~inside)
    for w in ("uniform", "cotangent"):
        assert torch.equal(meshing.smooth_mesh(vt, ft, weights=w)[border], vt[border])
        assert float((meshing.smooth_mesh(vt, ft, weights=w, boundary="free")[border] - vt[border]).abs().max()) > 1e-3
    assert torch.equal(meshing.denoise_mesh(vt, ft)[0][border], vt[border])
    assert float((meshing.denoise_mesh(vt, ft, boundary="free")[0][border] - vt[border]).abs().max()) > 1e-4


def test_winding_does_not_matter_to_denoise_mesh():
    from neuraludf_amd import meshing
    v, f = MESHES["cube"]
    rng = np.random.default_rng(3)
    flip = rng.random(len(f)) < 0.5
    g = f.copy()
    g[flip] = g[flip][:, [0, 2, 1]]
    pa, na = meshing.denoise_mesh(_dev(v), _dev(f))
    pb, nb = meshing.denoise_mesh(_dev(v), _dev(g))
    assert 0 < flip.sum() < len(f) and torch.equal(pa, pb)
    assert torch.equal(torch.where(_dev(flip)[:, None], -nb, nb), na)


def test_nothing_to_do_two_runs_and_float32():
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    vt, ft = _dev(v), _dev(f)
    assert torch.equal(meshing.smooth_mesh(vt, ft, 0), vt)
    pos, fn = meshing.denoise_mesh(vt, ft, 0, 0)
    assert torch.equal(pos, vt)
    np.testing.assert_array_equal(fn.cpu().numpy(), S.frames(v, f)[0])        # the input's own normals
    for w in ("uniform", "cotangent"):
        assert torch.equal(meshing.smooth_mesh(vt, ft, weights=w), meshing.smooth_mesh(vt, ft, weights=w))
    a, b = meshing.denoise_mesh(vt, ft), meshing.denoise_mesh(vt, ft)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    v32 = vt.float()
    out = meshing.smooth_mesh(v32, ft)
    assert out.dtype == torch.float32
    np.testing.assert_array_equal(out.cpu().numpy(), S.smooth_mesh(v.astype(np.float32), f))
    pos, fn = meshing.denoise_mesh(v32, ft)
    assert pos.dtype == fn.dtype == torch.float32 and pos.shape == v32.shape
    empty = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    assert meshing.smooth_mesh(vt, empty) is vt or torch.equal(meshing.smooth_mesh(vt, empty), vt)
    pos, fn = meshing.denoise_mesh(vt, empty)
    assert torch.equal(pos, vt) and fn.shape == (0, 3)


def test_argument_errors():
    from neuraludf_amd import meshing
    v, f = MESHES["three"]
    vt, ft = _dev(v), _dev(f)
    for bad in (dict(iterations=-1), dict(iterations=1.5), dict(lam=float("nan")), dict(mu=float("inf")),
                dict(weights="cot"), dict(boundary="open"), dict(fixed=torch.zeros(3, dtype=torch.bool, device=DEV)),
                dict(fixed=torch.zeros((len(v), 1), dtype=torch.bool, device=DEV))):
        with pytest.raises(ValueError):
            meshing.smooth_mesh(vt, ft, **bad)
    for bad in (dict(normal_iterations=-1), dict(vertex_iterations=-2), dict(sigma_s=0.0), dict(sigma_s=float("nan")),
                dict(sigma_c=-1.0), dict(sigma_c=float("inf")), dict(boundary="open"),
                dict(fixed=torch.zeros(2, dtype=torch.bool, device=DEV))):
        with pytest.raises(ValueError):
            meshing.denoise_mesh(vt, ft, **bad)
    with pytest.raises(ValueError):
        meshing.smooth_mesh(vt.cpu(), ft.cpu())


def test_sphere_keeps_its_radius():
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    vt, ft = _dev(v), _dev(f)
    rms0, _ = S.radial_stats(v)
    rms, radius = S.radial_stats(meshing.smooth_mesh(vt, ft, 10, 0.5, -0.53).cpu().numpy())
    print(f"sphere: RMS radial error {rms0:.5f} -> Taubin {rms:.5f}, mean radius {radius:.5f}")
    assert rms < 0.6 * rms0 and abs(radius - 1.0) < 0.005
    shrunk = S.radial_stats(meshing.smooth_mesh(vt, ft, 10, 0.5, 0.0).cpu().numpy())[1]
    assert shrunk < 0.96
    rms, radius = S.radial_stats(meshing.denoise_mesh(vt, ft)[0].cpu().numpy())
    print(f"sphere: plain Laplacian mean radius {shrunk:.5f}; denoise_mesh RMS {rms:.5f}, mean radius {radius:.5f}")
    assert rms < 0.4 * rms0 and abs(radius - 1.0) < 0.001


def test_cube_keeps_its_edges():
    from neuraludf_amd import meshing
    v, f, side = S.noisy_cube()
    vt, ft = _dev(v), _dev(f)
    before = S.mean_normal_angle(S.frames(v, f)[0], side)
    out, fn = meshing.denoise_mesh(vt, ft)
    after = S.mean_normal_angle(S.frames(out.cpu().numpy(), f)[0], side)
    taubin = S.mean_normal_angle(S.frames(meshing.smooth_mesh(vt, ft).cpu().numpy(), f)[0], side)
    print(f"cube: mean normal angle {before:.2f} -> denoise_mesh {after:.2f}, Taubin {taubin:.2f} degrees")
    assert after < 2.0 and after < before / 3.0 and taubin > before


@pytest.mark.parametrize("weights", ["uniform", "cotangent"])
def test_sheet_noise_is_halved(weights):
    from neuraludf_amd import meshing
    v, f, inside = S.noisy_sheet()
    out = meshing.smooth_mesh(_dev(v), _dev(f), weights=weights).cpu().numpy()
    rms0, rms = (float(np.sqrt(np.mean(x[inside, 2] ** 2))) for x in (v, out))
    print(f"sheet, {weights}: interior RMS height {rms0:.5f} -> {rms:.5f}")
    assert rms < 0.5 * rms0


# ---- wiring ------------------------------------------------------------------------------------------------------------
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


def test_extract_udf_mesh_filters_before_it_simplifies():
    from neuraludf_amd import meshing
    udf = _SphereUDF(0.6).to(DEV)
    n = 33
    cell = 2.0 * meshing.grid_spacing(*BOX, n)
    v0, f0 = meshing.extract_udf_mesh(udf, n, keep_largest=True)
    vt, ft = _dev(v0), _dev(f0)
    den = meshing.denoise_mesh(vt, ft)[0]
    both = meshing.smooth_mesh(den, ft, 3)
    v1, f1 = meshing.extract_udf_mesh(udf, n, keep_largest=True, denoise=True)
    np.testing.assert_array_equal(v1, den.cpu().numpy())
    np.testing.assert_array_equal(f1, f0)
    v2, f2 = meshing.extract_udf_mesh(udf, n, keep_largest=True, smooth=3, denoise=True)
    np.testing.assert_array_equal(v2, both.cpu().numpy())
    assert v2.dtype == np.float32 and np.abs(v2 - v0).max() > 1e-5
    args = dict(iterations=2, weights="cotangent", boundary="free")
    v3, _ = meshing.extract_udf_mesh(udf, n, keep_largest=True, smooth=args)
    np.testing.assert_array_equal(v3, meshing.smooth_mesh(vt, ft, **args).cpu().numpy())
    want = meshing.simplify_mesh(both, ft, cell)
    v4, f4 = meshing.extract_udf_mesh(udf, n, keep_largest=True, smooth=3, denoise=True, simplify_cell=cell)
    np.testing.assert_array_equal(v4, want.verts.cpu().numpy())
    np.testing.assert_array_equal(f4, want.faces.cpu().numpy())


def test_cli_round_trip_keeps_the_colours(tmp_path, capsys):
    from neuraludf_amd import meshing
    v, f = MESHES["sphere"]
    v32 = v.astype(np.float32)
    colours = np.random.default_rng(1).integers(0, 256, (len(v), 3)).astype(np.uint8)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    meshing.write_ply(src, v32, f, colors=colours)
    assert meshing.main([src, dst, "--smooth", "4"]) == 0
    ov, of, oc = meshing.read_ply(dst, with_colors=True)
    np.testing.assert_array_equal(ov, S.smooth_mesh(v32, f, 4))
    np.testing.assert_array_equal(of, f)
    np.testing.assert_array_equal(oc, colours)
    assert meshing.main([src, dst, "--smooth", "2", "--smooth-weights", "cotangent", "--free-boundary"]) == 0
    ov, _, oc = meshing.read_ply(dst, with_colors=True)
    np.testing.assert_array_equal(ov, S.smooth_mesh(v32, f, 2, weights="cotangent", boundary="free"))
    np.testing.assert_array_equal(oc, colours)
    assert meshing.main([src, dst, "--denoise", "--sigma-s", "0.3", "--smooth", "1"]) == 0
    ov, of, oc = meshing.read_ply(dst, with_colors=True)
    rv, rf, _ = meshing.read_ply(src, with_colors=True)                        # in the reader's dtype, as the CLI holds it
    vt, ft = _dev(rv), _dev(rf)
    want = meshing.smooth_mesh(meshing.denoise_mesh(vt, ft, sigma_s=0.3)[0], ft, 1)
    np.testing.assert_array_equal(ov, want.cpu().numpy().astype(np.float32))   # the file holds float32
    np.testing.assert_array_equal(oc, colours)
    assert meshing.main([src, dst]) == 0                                       # no switch: as before
    sv, _, sc = meshing.read_ply(dst, with_colors=True)
    np.testing.assert_array_equal(sv, v32)
    assert sc is None
    with pytest.raises(SystemExit):
        meshing.main([src, dst, "--smooth-weights", "area"])
