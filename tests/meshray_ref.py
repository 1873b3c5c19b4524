"""The numpy restatement of csrc/meshray.hip's per-(ray, face) rule: brute force over all faces, chunked
over the rays, no grid; every float64 product, sum and quotient in the kernel's order (numpy fuses nothing).  The GPU
results must equal it bit for bit; tests/test_meshray_ref.py holds it to things it was not built from.

The rule.  Axes are permuted so that z is the axis of the largest |d| (the lowest on a tie), x and y the next two
cyclically.  S = (d_x / d_z, d_y / d_z, 1 / d_z).  The corners are taken in ascending vertex index (A, B, C; equal
indices keep their corner order); each becomes P = V - o, then (P_x - S_x P_z, P_y - S_y P_z, S_z P_z).  The three edge
functions are evaluated once each, from the lower index to the higher, E(P, Q) = P_x Q_y - P_y Q_x:
w_A = E(B, C), w_B = -E(A, C), w_C = E(A, B); det = (w_A + w_B) + w_C; t = ((w_A A_z + w_B B_z) + w_C C_z) / det; the
weights are w / det, handed back at the face's own corners.  A face is hit when det != 0, t_min <= t <= t_max, t < inf
and
    first / any:  all three w >= 0 or all three w <= 0;
    count:        the three signs agree, a zero counting as positive in the edge's own direction (so E(A, C) == 0 makes
                  w_B negative).
A face with an index out of range or a non-finite vertex is absent."""
import numpy as np

INF = np.inf
MODES = ("first", "any", "count")


def usable_faces(verts, faces):
    """[F] bool: every index in range and every coordinate finite"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    ok[ok] = np.isfinite(verts[faces[ok]]).all((1, 2))
    return ok


def dominant_axis(d):
    """[Q] the axis of the largest |d|, the lowest on a tie"""
    a = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    m = a[:, 0]
    t = a[:, 1] > m
    kz[t], m = 1, np.where(t, a[:, 1], m)
    kz[a[:, 2] > m] = 2
    return kz


def face_hits(o, d, verts, faces, t_min=0.0, t_max=INF):
    """rays [Q, 3] against every face -> (t [Q, F], w [Q, F, 3] at the face's corners, inclusive [Q, F] bool,
    crossing [Q, F] bool); t_min / t_max scalars or [Q]"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    Q, F = len(o), len(faces)
    ok = usable_faces(verts, faces)
    fi = np.where(ok[:, None], faces, 0)
    order = np.argsort(fi, axis=1, kind="stable")                  # order[f, k] = the corner of the k-th lowest index
    VS = np.where(ok[:, None, None], verts[fi], 0.0)               # [F, corner, 3]
    kz = dominant_axis(d)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(Q)
    t_min = np.broadcast_to(np.asarray(t_min, np.float64), (Q,))[:, None]
    t_max = np.broadcast_to(np.asarray(t_max, np.float64), (Q,))[:, None]
    with np.errstate(all="ignore"):
        dz = d[rows, kz]
        Sx, Sy, Sz = (d[rows, kx] / dz)[:, None], (d[rows, ky] / dz)[:, None], (1.0 / dz)[:, None]
        P = []
        for k in range(3):
            rel = VS[np.arange(F), order[:, k]][None] - o[:, None, :]                  # [Q, F, 3]
            rx, ry, rz = (np.take_along_axis(rel, np.broadcast_to(a[:, None, None], (Q, F, 1)), 2)[..., 0]
                          for a in (kx, ky, kz))
            P.append((rx - Sx * rz, ry - Sy * rz, Sz * rz))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = P
        cBC = Bx * Cy - By * Cx
        cAC = Ax * Cy - Ay * Cx
        cAB = Ax * By - Ay * Bx
        wA, wB, wC = cBC, -cAC, cAB
        det = (wA + wB) + wC
        t = ((wA * Az + wB * Bz) + wC * Cz) / det
        ws = np.stack([wA / det, wB / det, wC / det], -1)
        w = np.take_along_axis(ws, np.broadcast_to(np.argsort(order, axis=1)[None], (Q, F, 3)), 2)
        valid = ok[None] & (det != 0) & (t >= t_min) & (t <= t_max) & (t < INF)
        inclusive = valid & (((wA >= 0) & (wB >= 0) & (wC >= 0)) | ((wA <= 0) & (wB <= 0) & (wC <= 0)))
        pA, pB, pC = cBC >= 0, ~(cAC >= 0), cAB >= 0
        crossing = valid & (pA == pB) & (pB == pC)
    return t, w, inclusive, crossing


def cast(origins, directions, verts, faces, t_min=0.0, t_max=INF, mode="first", chunk=256):
    """first -> (t [N], face [N] int64, bary [N, 3]): the smallest (t, face), +inf / -1 / NaN on a miss;
    any -> [N] bool; count -> [N] int64"""
    assert mode in MODES
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    N = len(o)
    t_min = np.broadcast_to(np.asarray(t_min, np.float64), (N,))
    t_max = np.broadcast_to(np.asarray(t_max, np.float64), (N,))
    ts, face, bary = np.full(N, INF), np.full(N, -1, np.int64), np.full((N, 3), np.nan)
    anyhit, count = np.zeros(N, bool), np.zeros(N, np.int64)
    for b in range(0, N, chunk):
        s = slice(b, b + chunk)
        t, w, inc, cro = face_hits(o[s], d[s], verts, faces, t_min[s], t_max[s])
        if mode == "count":
            count[s] = cro.sum(1)
            continue
        anyhit[s] = inc.any(1)
        tm = np.where(inc, t, INF)
        f = np.argmin(tm, 1)                           # the first minimum: the lowest face index
        rows = np.arange(len(f))
        sel = np.nonzero(tm[rows, f] < INF)[0]
        ts[b + sel], face[b + sel], bary[b + sel] = tm[sel, f[sel]], f[sel], w[sel, f[sel]]
    if mode == "count":
        return count
    if mode == "any":
        return anyhit
    return ts, face, bary


def parity_inside(points, verts, faces, directions):
    """crossing parity of the rays from `points` along each of `directions` [K, 3], the majority over K (odd)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    votes = np.zeros(len(p), np.int64)
    for dk in np.asarray(directions, np.float64):
        votes += cast(p, np.broadcast_to(dk, p.shape), verts, faces, mode="count") & 1
    return 2 * votes > len(directions)


# ---- the meshes the CPU and GPU tests share -------------------------------------------------------------------------
def icosphere(subdivisions=2, radius=1.0):
    """320 faces at two subdivisions, wound outward"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return radius * np.array(v), np.array(f, np.int64)


def grid_sheet(n, fn=None, flip_odd=False):
    """n x n quads over [0, 1]^2 with spacing 1 / n (exactly representable for n a power of two), z = fn(x, y);
    flip_odd winds the second triangle of every quad the other way"""
    k = np.arange(n + 1) / n
    x, y = np.meshgrid(k, k, indexing="ij")
    z = np.zeros_like(x) if fn is None else fn(x, y)
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    f = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            f += [[a, b, c], [a, d, c] if flip_odd else [a, c, d]]
    return v, np.array(f, np.int64)


def folded_sheet():
    """8 x 8 quads folded along x = 0.5 and rippled, so that a ray can cross it several times"""
    v, f = grid_sheet(8, lambda x, y: 0.9 * np.abs(x - 0.5) + 0.05 * np.sin(7.0 * y))
    return v - np.array([0.5, 0.5, 0.2]), f


def cube():
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, np.int64)
