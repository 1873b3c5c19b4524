"""The "hostile" mesh the poisoned-allocation tests of the mesh tools share (tests/test_gpu_mesh_poison.py), numpy only: an
icosphere subdivided twice (162 vertices, 320 faces) with the face fan of one vertex removed (a border loop; the vertex stays,
unreferenced), a detached triangle (a second component), a zero-area face whose two coinciding corners differ in index (a
third component), and one more unreferenced vertex.  Built in float64 from a fixed seed; tests/test_mesh_poison_cases.py
checks on the CPU that it is what it says."""
import functools

import numpy as np

FAN_VERTEX = 7


@functools.lru_cache(maxsize=None)
def hostile():
    """-> (verts [V, 3] float64, faces [F, 3] int64, dict of the indices of its parts); read only"""
    import meshray_ref
    v, f = meshray_ref.icosphere(2)
    assert v.shape == (162, 3) and f.shape == (320, 3)
    rng = np.random.default_rng(20251)
    v = 0.6 * v + rng.normal(scale=0.003, size=v.shape)
    fan = (f == FAN_VERTEX).any(1)
    f = f[~fan]
    n = len(v)
    extra = np.array([[0.86, 0.05, 0.02], [0.97, 0.08, 0.05], [0.9, 0.17, -0.03],          # n .. n+2: the detached triangle
                      [-0.85, 0.1, 0.2], [-0.85, 0.1, 0.2], [-0.8, 0.22, 0.25],             # n+3 .. n+5: the zero-area face
                      [0.1, -0.9, 0.3]])                                                    # n+6: unreferenced
    more = np.array([[n, n + 1, n + 2], [n + 3, n + 4, n + 5]], dtype=np.int64)
    verts = np.ascontiguousarray(np.concatenate([v, extra]), dtype=np.float64)
    faces = np.ascontiguousarray(np.concatenate([f, more]), dtype=np.int64)
    verts.setflags(write=False)
    faces.setflags(write=False)
    parts = dict(fan_faces=int(fan.sum()), detached=len(faces) - 2, zero_area=len(faces) - 1, unreferenced=(FAN_VERTEX, n + 6),
                 n_sphere_verts=n)
    return verts, faces, parts
