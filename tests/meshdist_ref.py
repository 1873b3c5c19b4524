"""The numpy restatement of csrc/meshdist.hip's per-face rule: brute force over all faces, chunked over
the queries, every float64 product, sum, quotient and square root in the kernel's order (numpy fuses nothing).  The GPU
results must equal it bit for bit; tests/test_meshdist_ref.py holds it to things it was not built from."""
import numpy as np

INF = np.inf


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def usable_faces(verts, faces):
    """[F] bool: every index in range and every coordinate finite (the faces the index bins)"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    ok[ok] = np.isfinite(verts[faces[ok]]).all((1, 2))
    return ok


def _better(d2, c, w, best):
    """replace where strictly closer (a NaN never is)"""
    with np.errstate(invalid="ignore"):
        take = d2 < best[0]
    best[0] = np.where(take, d2, best[0])
    best[1] = np.where(take[..., None], c, best[1])
    best[2] = np.where(take[..., None], w, best[2])


def face_candidates(p, verts, faces):
    """p [Q, 3] against every face -> (d2 [Q, F], c [Q, F, 3], w [Q, F, 3]); d2 = +inf for an absent face"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    ok = usable_faces(verts, faces)
    fi = np.where(ok[:, None], faces, 0)
    V = [np.where(ok[:, None], verts[fi[:, k]], 0.0)[None] for k in range(3)]          # [1, F, 3] each
    P = p[:, None, :]
    Q, F = len(p), len(faces)
    best = [np.full((Q, F), INF), np.full((Q, F, 3), INF), np.zeros((Q, F, 3))]
    with np.errstate(all="ignore"):
        # interior, on the corners in ascending vertex index (A, B, C): no bit depends on the winding
        order = np.argsort(fi, axis=1, kind="stable")                 # order[f, k] = the corner of the k-th lowest index
        VS = np.stack([V[0][0], V[1][0], V[2][0]], 1)                 # [F, corner, 3]
        A, B, C = (VS[np.arange(F), order[:, k]][None] for k in range(3))
        n = _cross(B - A, C - A)
        nn = _dot(n, n)
        sa = _dot(_cross(C - B, P - B), n)
        sb = _dot(_cross(A - C, P - C), n)
        sc = _dot(_cross(B - A, P - A), n)
        inside = (nn > 0) & (nn < INF) & (sa > 0) & (sb > 0) & (sc > 0)
        h = _dot(P - A, n) / nn
        hn = h[..., None] * n
        s = (sa + sb) + sc
        d2 = np.where(inside, _dot(hn, hn), INF)
        ws = np.stack([sa / s, sb / s, sc / s], -1)
        w = np.take_along_axis(ws, np.argsort(order, axis=1)[None], 2)          # back to the face's corner order
        _better(d2, P - hn, w, best)
        # edges, each from its lower vertex index to its higher
        for ka, kb in ((0, 1), (1, 2), (2, 0)):
            swap = (fi[:, ka] > fi[:, kb])[None, :, None]
            a, b = np.where(swap, V[kb], V[ka]), np.where(swap, V[ka], V[kb])
            e = b - a
            ee = _dot(e, e)
            t = np.where(ee == 0, 0.0, _dot(P - a, e) / np.where(ee == 0, 1.0, ee))
            lo, hi = (t <= 0)[..., None], (t >= 1)[..., None]
            c = np.where(lo, a, np.where(hi, b, a + t[..., None] * e))
            wa = np.where(lo[..., 0], 1.0, np.where(hi[..., 0], 0.0, 1.0 - t))
            wb = np.where(lo[..., 0], 0.0, np.where(hi[..., 0], 1.0, t))
            r = P - c
            w = np.zeros((Q, F, 3))
            sw = swap[..., 0]
            w[..., ka] = np.where(sw, wb, wa)
            w[..., kb] = np.where(sw, wa, wb)
            _better(_dot(r, r), c, w, best)
    best[0] = np.where(ok[None, :], best[0], INF)
    return best


def closest(query, verts, faces, bound=INF, chunk=256):
    """-> (dist [M], face [M] int64, point [M, 3], bary [M, 3]): the smallest (d2, face) over all faces; beyond bound
    +inf, -1, NaN, NaN"""
    query = np.asarray(query, np.float64).reshape(-1, 3)
    M = len(query)
    dist, face = np.full(M, INF), np.full(M, -1, np.int64)
    point, bary = np.full((M, 3), np.nan), np.full((M, 3), np.nan)
    for b in range(0, M, chunk):
        d2, c, w = face_candidates(query[b:b + chunk], verts, faces)
        f = np.argmin(d2, 1)                       # the first minimum: the lowest face index
        rows = np.arange(len(f))
        m = d2[rows, f]
        d = np.sqrt(m)
        hit = (m < INF) & (d <= bound)
        sel = np.nonzero(hit)[0]
        dist[b + sel], face[b + sel] = d[sel], f[sel]
        point[b + sel], bary[b + sel] = c[sel, f[sel]], w[sel, f[sel]]
    return dist, face, point, bary
