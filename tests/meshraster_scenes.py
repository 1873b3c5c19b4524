"""The small scenes the rasteriser's CPU and GPU tests share (tests/test_meshraster_ref.py, tests/test_gpu_meshraster.py):
pinhole cameras, squares and sheets, all float64 numpy.  Imported by the tests only."""
import numpy as np


def pinhole(f, cx, cy, R=None, C=None):
    """world matrix [4, 4] of a pinhole camera at C looking along the rows of R: P = K [R | -R C]"""
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    C = np.zeros(3) if C is None else np.asarray(C, dtype=np.float64)
    P = np.eye(4)
    P[:3, :3] = K @ R
    P[:3, 3] = -(K @ R) @ C
    return P


REAR = np.diag([-1.0, 1.0, -1.0])        # a camera turned by 180 degrees about the image's vertical axis


def square(half, z, first=0):
    """a fronto-parallel square of two triangles sharing the diagonal from its first to its third vertex"""
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], dtype=np.float64)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64) + first


# 32 x 24 image, focal length 16: the square of half-size 1 at depth 2 lands exactly on the pixels [8, 24] x [4, 20], the one
# of half-size 1/4 at depth 1 on [12, 20] x [8, 16]; both areas are powers of two, so the barycentrics are exact
SQ_W, SQ_H = 32, 24
SQ_P = pinhole(16.0, 16.0, 12.0)[None]


def two_squares():
    v0, f0 = square(1.0, 2.0)
    v1, f1 = square(0.25, 1.0, first=4)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1])


def sheet(n, fn):
    """an n x n sheet of 2 n^2 triangles over (u, v) in [-1, 1]^2, vertex (u, v) at fn(u, v) -> (verts, faces)"""
    t = np.linspace(-1.0, 1.0, n + 1)
    u, v = np.meshgrid(t, t, indexing="xy")
    verts = np.stack(fn(u.reshape(-1), v.reshape(-1)), -1).astype(np.float64)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    a = (j * (n + 1) + i).reshape(-1)
    faces = np.concatenate([np.stack([a, a + 1, a + n + 2], -1), np.stack([a, a + n + 2, a + n + 1], -1)])
    return verts, faces.astype(np.int64)


def tilted_sheet(degrees, n=20):
    """a plane through (0, 0, 3) turned by `degrees` about the image's vertical axis: depths within 2 .. 4"""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return sheet(n, lambda u, v: (u * c, v, 3.0 + u * s))


def ridge_sheet(n=20):
    """the sheet folded along u = 0 into a ridge that points at the camera: depths 2 (the crease) .. 2 + sin 45"""
    c = s = np.sqrt(0.5)
    return sheet(n, lambda u, v: (u * c, v, 2.0 + np.abs(u) * s))


VIS_W, VIS_H = 64, 48
VIS_P = pinhole(60.0, 32.0, 24.0)[None]
VIS_GAP = 1e-5


def parallel_sheets(n=10):
    """a front sheet at z = 2 and a back sheet at z = 3 (both of half-size 1), a front camera at the origin and a rear
    one at (0, 0, 5) looking back: each camera's near sheet covers the far one -> (verts, faces, world_mats, n_front)"""
    v0, f0 = sheet(n, lambda u, v: (u, v, 2.0 + 0 * u))
    v1, f1 = sheet(n, lambda u, v: (u, v, 3.0 + 0 * u))
    mats = np.stack([pinhole(40.0, 32.0, 24.0), pinhole(40.0, 32.0, 24.0, REAR, (0.0, 0.0, 5.0))])
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]), mats, len(v0)


RAG_W, RAG_H = 65, 33


def ragged():
    """a wavy 20 x 20 sheet seen by three cameras, plus: one triangle spanning most of the image (behind the sheet), a face
    with a vertex behind the first two cameras, a face partly outside the image, a zero-area face, a face repeating a
    vertex, and a face with a NaN vertex -> (verts, faces, world_mats, expected skipped count)"""
    verts, faces = sheet(20, lambda u, v: (0.8 * u, 0.45 * v, 3.0 + 0.2 * np.sin(3.0 * u) * np.cos(2.0 * v) + 0.3 * u))
    n = len(verts)
    extra = np.array([
        [-2.4, -1.2, 4.5], [2.4, -1.1, 4.5], [0.1, 1.3, 4.4],          # n .. n+2: the large triangle
        [0.2, 0.1, 2.0], [0.3, 0.1, 2.0], [0.6, 0.5, -0.7],            # n+3 .. n+5: the last one behind cameras 0 and 1
        [1.0, 0.5, 2.5], [1.6, 0.55, 2.5], [1.2, 0.9, 2.6],            # n+6 .. n+8: partly outside
        [0.0, 0.0, 2.0], [0.25, 0.25, 2.0], [0.5, 0.5, 2.0],           # n+9 .. n+11: collinear, area exactly 0 in view 0
        [np.nan, 0.0, 2.0],                                            # n+12
    ])
    more = np.array([[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n + 6, n + 7, n + 8], [n + 9, n + 10, n + 11],
                     [n + 3, n + 4, n + 3], [n + 3, n + 12, n + 4]], dtype=np.int64)
    c, s = np.cos(0.3), np.sin(0.3)
    mats = np.stack([
        pinhole(40.0, 32.0, 16.0),
        pinhole(37.3, 30.2, 17.1, [[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]], (0.9, 0.1, 0.2)),
        pinhole(35.0, 33.0, 15.5, REAR, (0.1, 0.0, 6.0)),
    ])
    # skipped: the NaN face in all three views, the face with a vertex behind the camera in the first two
    return np.concatenate([verts, extra]), np.concatenate([faces, more]), mats, 5
