"""The hand-built meshes of the hole-closing tests (tests/test_meshhole_ref.py on the CPU, tests/test_gpu_meshhole.py on the
GPU): numpy only.  A grid of nx x ny quads, each split (v00, v10, v11), (v00, v11, v01); holes are quads and triangles left
out.  Every case is (verts [V, 3] float64, faces [F, 3] int64)."""
import numpy as np


def grid(nx, ny, skip_quads=(), skip_b=(), skip_a=(), height=None):
    """skip_quads: quads left out whole; skip_b / skip_a: quads whose second / first triangle is left out"""
    vid = lambda x, y: y * (nx + 1) + x
    xs, ys = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64))
    z = np.zeros_like(xs) if height is None else height(xs, ys)
    verts = np.stack([xs.reshape(-1), ys.reshape(-1), z.reshape(-1)], 1)
    skip_quads, skip_a, skip_b = set(skip_quads), set(skip_a), set(skip_b)
    faces = []
    for y in range(ny):
        for x in range(nx):
            if (x, y) in skip_quads:
                continue
            if (x, y) not in skip_a:
                faces.append((vid(x, y), vid(x + 1, y), vid(x + 1, y + 1)))
            if (x, y) not in skip_b:
                faces.append((vid(x, y), vid(x + 1, y + 1), vid(x, y + 1)))
    return verts, np.array(faces, np.int64)


def _bump(xs, ys):
    return 0.3 * np.sin(0.9 * xs + 0.2) * np.cos(0.7 * ys - 0.4) + 0.05 * xs * ys / 10.0


def annulus(k, saddle=0.0, seed=0):
    """a ring of 2 k triangles around a k-gon hole: two closed loops of k edges, neither planar"""
    rng = np.random.default_rng(seed + k)
    t = 2 * np.pi * np.arange(k) / k
    inner = np.stack([np.cos(t), np.sin(t), saddle * np.cos(2 * t) + 0.1 * rng.standard_normal(k)], 1)
    outer = np.stack([2.5 * np.cos(t + 0.2), 2.5 * np.sin(t + 0.2), 0.3 * rng.standard_normal(k)], 1)
    faces = []
    for i in range(k):
        j = (i + 1) % k
        faces += [(i, k + i, k + j), (i, k + j, j)]
    return np.concatenate([inner, outer]), np.array(faces, np.int64)


def block(x0, y0, w, h, extra=0):
    """the quads of a w x h block and `extra` second-triangles of the quads on its right side: a hole of 2 (w + h) + extra
    edges"""
    return [(x, y) for x in range(x0, x0 + w) for y in range(y0, y0 + h)], [(x0 + w, y0 + i) for i in range(extra)]


def bow_tie(k1=4, k2=5):
    """two holes that share one vertex: two rings (annulus) whose inner rims of k1 and k2 edges meet in the first's vertex 0
    and nowhere else.  That vertex has four border edges, so a rule by border degree gives up there and a cycle basis may
    pair the edges either way; the two fans around it say which belong together: four closed loops k1, k1, k2, k2.  (The
    second ring's own vertex 0 stays in the table, unreferenced.)"""
    va, fa = annulus(k1)
    vb, fb = annulus(k2, seed=7)
    vb = 2 * va[0] - (vb + (va[0] - vb[0]))                     # moved onto the shared vertex and mirrored through it
    fb = fb + len(va)
    fb[fb == len(va)] = 0
    return np.concatenate([va, vb]), np.concatenate([fa, fb])


def shared_diagonal():
    """two rings whose 4-gon inner rims share the two opposite vertices p = 0 and q = 2 and nothing else; both rims are
    folded along p-q (their other two vertices lie one above, the other's one below the plane), so the minimum-area
    triangulation of each takes the diagonal p-q: the second patch would put four faces on that edge"""
    t = 2 * np.pi * np.arange(4) / 4
    outer = np.stack([2.5 * np.cos(t + 0.2), 2.5 * np.sin(t + 0.2), np.zeros(4)], 1)
    inner = np.array([[0.5, 0.0, 0.0], [0.0, 1.0, 1.0], [-0.5, 0.0, 0.0], [0.0, -1.0, 1.0]])
    ring = annulus(4)[1]                                        # inner 0 ... 3, outer 4 ... 7
    second = np.array([0, 8, 2, 9, 10, 11, 12, 13])[ring]       # p and q shared, the rest its own
    verts = np.concatenate([inner, outer, inner[[1, 3]] * [1, 1, -1], outer + [0.0, 0.0, -3.0]])
    return verts, np.concatenate([ring, second])


def pinched_holes():
    """two 4-holes at opposite corners of the vertex (2, 2) of a 5 x 5 grid.  The surface around that vertex is two wedges,
    each between one hole and the other, so the fans lead from the rim of one hole to the rim of the other: one closed loop
    of 8 edges that passes the vertex twice, and the outer border of 20"""
    return grid(5, 5, skip_quads=[(1, 1), (2, 2)], height=_bump)


def fin():
    """a 4-hole at quad (1, 1) of a 5 x 5 grid and a third face on the edge (1, 1)-(0, 1) that leaves its corner: the fans
    around both ends of that edge are blocked, so the hole, the fin and the outer border are open chains"""
    verts, faces = grid(5, 5, skip_quads=[(1, 1)], height=_bump)
    a, b = 1 * 6 + 1, 1 * 6 + 0
    verts = np.concatenate([verts, [[0.5, 1.0, 1.0]]])
    return verts, np.concatenate([faces, [[a, b, len(verts) - 1]]])


def repeated_vertex_face():
    """the 4-hole at quad (1, 1) with a face (a, a, b) on its rim edge a-b: that edge has three half-edges now and blocks,
    and the face's own edge a-a is a chain of one edge"""
    verts, faces = grid(5, 5, skip_quads=[(1, 1)], height=_bump)
    a, b = 1 * 6 + 1, 1 * 6 + 2
    return verts, np.concatenate([faces, [[a, a, b]]])


def strip_over_hole():
    """the 4-hole at quad (2, 2) of a 5 x 5 grid with two far faces over its diagonals: whichever the triangulation picks is
    an edge already.  Each far face is the border of itself besides: a 3-loop whose triangle is a face"""
    verts, faces = grid(5, 5, skip_quads=[(2, 2)], height=_bump)
    a, b, c, d = 2 * 6 + 2, 2 * 6 + 3, 3 * 6 + 3, 3 * 6 + 2
    verts = np.concatenate([verts, [[2.5, 2.5, 3.0], [2.5, 2.5, -3.0]]])
    return verts, np.concatenate([faces, [[a, c, len(verts) - 2], [b, d, len(verts) - 1]]])


SPHERE_HOLES = (3, 4, 5, 6, 7, 17, 63, 64, 65)


def sphere_patch(holes=SPHERE_HOLES):
    """a 60 x 28 grid on the unit sphere with one hole of each length punched into it; the holes sit on the sphere, so none
    is planar"""
    nx, ny = 60, 28
    quads, b_tris, a_tris = [], [], []
    big = iter([(2, 2), (21, 2), (40, 2)])
    small = iter([(8 + 5 * i, 21) for i in range(10)])
    for n in holes:
        if n == 3:
            x, y = next(small)
            a_tris.append((x, y))
            continue
        w, h = {4: (1, 1), 5: (1, 1), 6: (1, 2), 7: (1, 2), 17: (4, 4), 63: (15, 16), 64: (16, 16), 65: (16, 16)}[n]
        x, y = next(big) if n > 60 else ((2, 21) if n == 17 else next(small))
        q, t = block(x, y, w, h, n - 2 * (w + h))
        quads += q
        b_tris += t
    verts, faces = grid(nx, ny, quads, b_tris, a_tris)
    theta, phi = 0.3 + 1.4 * verts[:, 0] / nx, 0.5 + 1.3 * verts[:, 1] / ny
    return np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], 1), faces


def flip_half(faces):
    out = faces.copy()
    out[1::2] = out[1::2][:, [0, 2, 1]]
    return out


def border_count(faces, n_verts):
    a, b = faces.reshape(-1), np.roll(faces, -1, 1).reshape(-1)
    key = np.minimum(a, b) * n_verts + np.maximum(a, b)
    _, counts = np.unique(key, return_counts=True)
    return int((counts == 1).sum()), int((counts > 2).sum())


def euler(faces):
    a, b = faces.reshape(-1), np.roll(faces, -1, 1).reshape(-1)
    n = int(faces.max()) + 1
    return len(np.unique(faces)) - len(np.unique(np.minimum(a, b) * n + np.maximum(a, b))) + len(faces)
