"""tests/mesh_poison_cases.py on the CPU: the hostile mesh has the parts its users rely on."""
import numpy as np

from mesh_poison_cases import hostile


def test_the_hostile_mesh_is_what_it_says():
    v, f, parts = hostile()
    assert len(v) == 169 and len(f) == 320 - parts["fan_faces"] + 2 and parts["fan_faces"] in (5, 6)
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    assert sorted(np.flatnonzero(~used).tolist()) == sorted(parts["unreferenced"])
    p = v[f]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert np.flatnonzero(area == 0).tolist() == [parts["zero_area"]]
    z = f[parts["zero_area"]]
    assert z[0] != z[1] and np.array_equal(v[z[0]], v[z[1]])
    import meshclean_ref
    labels = meshclean_ref.face_components(f, len(v))
    assert len(np.unique(labels)) == 3
    a, b = f.reshape(-1), np.roll(f, -1, 1).reshape(-1)
    _, counts = np.unique(np.minimum(a, b) * len(v) + np.maximum(a, b), return_counts=True)
    assert int((counts == 1).sum()) == parts["fan_faces"] + 6 and int((counts > 2).sum()) == 0
