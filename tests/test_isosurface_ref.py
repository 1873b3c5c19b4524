"""CPU: the numpy restatement of the level-set mesher (tests/isosurface_ref.py) on its own -- the generated case table
used for plain level sets gives closed, consistently wound surfaces of the right topology and measure."""
import math

import numpy as np

import isosurface_ref as I
import meshudf_ref as R


def _mesh(F, level, n, box=I.BOX):
    return I.marching_cubes(np.asarray(F), level, I.grid_axes(n, *box))


def test_random_field_all_cases_closed_and_consistently_wound():
    n = 24
    F = I.random_field(n, 3, raise_boundary=True).numpy()
    case, _ = I.cell_cases(F, 0.5)
    assert len(np.unique(case)) == 256
    v, f = _mesh(F, 0.5, n)
    assert len(f) > 1000 and f.max() == len(v) - 1
    _, cnt = R.edge_counts(f)
    assert (cnt == 2).all()
    assert I.directed_edges_unique(f)


def test_sphere_sdf():
    n, radius = 64, 0.6
    v, f = _mesh(I.grid_values(I.sphere_sdf, n, *I.BOX), 0.0, n)
    h = 2.0 / (n - 1)
    assert R.is_closed_manifold(f) and I.directed_edges_unique(f)
    assert R.euler(len(v), f) == 2 and R.components(len(v), f) == 1
    area, vol = R.area(v, f), I.signed_volume(v, f)
    err = float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - radius).max())
    print(f"area ratio {area / (4 * math.pi * radius ** 2):.4f}, volume ratio {vol / (4 / 3 * math.pi * radius ** 3):.4f}, "
          f"radial error {err / h:.4f} h")
    assert abs(area / (4 * math.pi * radius ** 2) - 1) <= 0.01
    assert vol > 0 and abs(vol / (4 / 3 * math.pi * radius ** 3) - 1) <= 0.01
    assert err <= 0.05 * h


def test_shell_of_an_unsigned_field_is_two_spheres():
    n = 64
    v, f = _mesh(I.grid_values(I.shell_udf, n, *I.BOX), 0.05, n)
    assert R.is_closed_manifold(f)
    assert R.components(len(v), f) == 2 and R.euler(len(v), f) == 4


def test_non_finite_nodes_silence_exactly_the_cells_that_touch_them():
    n, level = 24, 0.5
    clean = I.random_field(n, 11).numpy()
    dirty = I.random_field_with_specials(n, 11, level).numpy()
    bad = ~np.isfinite(dirty)
    assert bad.sum() == 5
    m = n - 1
    touch = np.zeros((m, m, m), dtype=bool)
    for dx, dy, dz in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        touch |= bad[dx:dx + m, dy:dy + m, dz:dz + m]
    # the nodes set to exactly the level change their own cells: compare with the clean field carrying those too
    ref = np.where(bad, clean, dirty)
    _, nt_ref = I.cell_cases(ref, level)
    _, nt = I.cell_cases(dirty, level)
    assert (nt_ref[touch] > 0).sum() > 20                     # they would have emitted
    np.testing.assert_array_equal(nt, np.where(touch, 0, nt_ref))
    v, f = _mesh(dirty, level, n)
    assert len(f) == nt.sum() and np.isfinite(v).all()


def test_plane_at_a_level_on_grid_nodes_is_two_sheets():
    n, level = 17, 0.25                                       # nodes at multiples of 1/8: |z| = level at two node planes
    F = I.grid_values(I.plane_udf, n, *I.BOX).numpy()
    assert (F == np.float32(level)).sum() == 2 * n * n
    v, f = _mesh(F, level, n)
    assert len(f) == 2 * 2 * (n - 1) ** 2
    assert R.components(len(v), f) == 2
    assert set(np.unique(v[:, 2]).tolist()) == {-0.25, 0.25}
