"""A numpy float64 restatement of the texture atlas (include/nudf.h nudf_meshtexture_*, csrc/meshtexture.hip,
neuraludf_amd/meshrender.py texture_atlas): the layout with plain loops over faces and Morton indices, the bake and the
shade with the expressions of the header in its order, evaluated for all texels (pixels) at once -- numpy multiplies,
adds, divides and takes square roots of float64 arrays one correctly rounded operation per element, which is what the
kernels do with contraction off.  The projection, the depth test and the weighted sample are those of
tests/meshraster_ref.py (project, visible, colour), rewritten over arrays.  Imported by the tests only."""
import numpy as np

F64 = np.float64
K_MIN, K_MAX, GUTTER = 3, 12, 6


def even_bits(m):
    """the bits 0, 2, 4, ... of the integer m, packed"""
    x, bit = 0, 0
    while m:
        x |= (m & 1) << bit
        m >>= 2
        bit += 1
    return x


def lower_chart(s):
    return [(1, 1), (s - 4, 1), (1, s - 4)]


def upper_chart(s):
    return [(s - 2, s - 2), (4, s - 2), (s - 2, 4)]


def owner_half(li, lj, s):
    """0 for the lower chart of a cell of side s, 1 for the upper one"""
    return 0 if li + lj <= s - 1 else 1


def face_class(pos, tri, density):
    """-> (k, the corner opposite the longest edge)"""
    n_verts = len(pos)
    v0, v1, v2 = (int(x) for x in tri)
    if min(v0, v1, v2) < 0 or max(v0, v1, v2) >= n_verts:
        return K_MIN, 0
    p = [np.asarray(pos[v], dtype=F64) for v in (v0, v1, v2)]
    with np.errstate(all="ignore"):
        sq = []
        for c in range(3):                                       # edge c joins the two corners other than c
            d = p[(c + 1) % 3] - p[(c + 2) % 3]
            sq.append((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        first, longest = 0, sq[0]
        for c in (1, 2):
            if sq[c] > longest:
                first, longest = c, sq[c]
        if v0 == v1 or v1 == v2 or v0 == v2 or not all(np.isfinite(x) for x in sq):
            return K_MIN, first
        t = np.sqrt(longest) * F64(density)
    k = K_MIN
    while k < K_MAX and t > F64((1 << k) - GUTTER):
        k += 1
    return k, first


def layout(pos, faces, density):
    """-> dict(uv [F, 3, 2] float64, W, H, cell_face [n_cells, 2] int64, class_off, class_k, k [F])"""
    pos, faces = np.asarray(pos, dtype=F64), np.asarray(faces, dtype=np.int64)
    cls = [face_class(pos, tri, density) for tri in faces]
    order = sorted(range(len(faces)), key=lambda f: (-cls[f][0], f))
    class_k = sorted({k for k, _ in cls}, reverse=True)
    class_off, cell_face, uv = [0], [], np.zeros((len(faces), 3, 2))
    for k in class_k:
        members = [f for f in order if cls[f][0] == k]
        s = 1 << k
        for e in range((len(members) + 1) // 2):
            m0 = class_off[-1] + e * 4 ** k
            X, Y = even_bits(m0), even_bits(m0 >> 1)
            assert X % s == 0 and Y % s == 0
            pair = members[2 * e:2 * e + 2]
            cell_face.append(pair + [-1] * (2 - len(pair)))
            for f, chart in zip(pair, (lower_chart(s), upper_chart(s))):
                for t, (ci, cj) in enumerate(chart):             # chart corner t holds the face's corner first + t
                    uv[f, (cls[f][1] + t) % 3] = (X + ci, Y + cj)
        class_off.append(class_off[-1] + ((len(members) + 1) // 2) * 4 ** k)
    W = 1
    while W * W < class_off[-1]:
        W *= 2
    H = W // 2 if 0 < class_off[-1] <= W * W // 2 else W
    return dict(uv=uv, W=W, H=H, cell_face=np.asarray(cell_face, dtype=np.int64).reshape(-1, 2), class_off=tuple(class_off),
                class_k=tuple(class_k), k=np.asarray([k for k, _ in cls], dtype=np.int64))


def owners(lay, n_faces):
    """the owner face of every texel -> int64 [H, W], -1 where there is none: by Morton index, as the bake kernel"""
    W, H, off, ks = lay["W"], lay["H"], lay["class_off"], lay["class_k"]
    first_cell = np.cumsum([0] + [(off[c + 1] - off[c]) >> (2 * k) for c, k in enumerate(ks)])
    own = np.full((H, W), -1, dtype=np.int64)
    for m in range(W * H):
        i, j = even_bits(m), even_bits(m >> 1)
        assert i < W and j < H
        if m >= off[-1]:
            continue
        c = max(c for c in range(len(ks)) if off[c] <= m)
        k, r = ks[c], m - off[c]
        cell = first_cell[c] + (r >> (2 * k))
        local = r & ((1 << (2 * k)) - 1)
        f = lay["cell_face"][cell][owner_half(even_bits(local), even_bits(local >> 1), 1 << k)]
        if 0 <= f < n_faces:
            own[j, i] = f
    return own


def barycentrics(uv, x, y):
    """of the points (x, y) in the triangles uv [N, 3, 2] -> (b0, b1, b2)"""
    ax, ay = uv[:, 0, 0] - x, uv[:, 0, 1] - y
    bx, by = uv[:, 1, 0] - x, uv[:, 1, 1] - y
    cx, cy = uv[:, 2, 0] - x, uv[:, 2, 1] - y
    w0 = bx * cy - cx * by
    w1 = cx * ay - ax * cy
    w2 = ax * by - bx * ay
    s = (w0 + w1) + w2
    return w0 / s, w1 / s, w2 / s


def mix(b, x0, x1, x2):
    return (b[0] * x0 + b[1] * x1) + b[2] * x2


def length(n):
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def taps(u, w, H, W):
    """-> ((ya, xa), (ya, xb), (yb, xa), (yb, xb)) indices and the four weights of the bilinear sample at (u, w)"""
    fx0, fy0 = np.floor(u), np.floor(w)
    fx, fy = u - fx0, w - fy0
    xa = np.fmin(np.fmax(fx0, 0.0), W - 1).astype(np.int64)
    xb = np.fmin(np.fmax(fx0 + 1.0, 0.0), W - 1).astype(np.int64)
    ya = np.fmin(np.fmax(fy0, 0.0), H - 1).astype(np.int64)
    yb = np.fmin(np.fmax(fy0 + 1.0, 0.0), H - 1).astype(np.int64)
    gx, gy = 1.0 - fx, 1.0 - fy
    return ((ya, xa), (ya, xb), (yb, xa), (yb, xb)), (gx * gy, fx * gy, gx * fy, fx * fy)


def seen(s, depth, min_gap):
    """the depth test of `visible` on the projections s [N, 3] against one depth map -> bool [N]"""
    H, W = depth.shape
    ok = np.isfinite(s).all(1) & (s[:, 2] > 0) & (np.abs(s[:, 0]) < 2.0 ** 52) & (np.abs(s[:, 1]) < 2.0 ** 52)
    px, py = np.rint(s[:, 0]), np.rint(s[:, 1])
    ok &= (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    ix, iy = np.where(ok, px, 0).astype(np.int64), np.where(ok, py, 0).astype(np.int64)
    m = np.full(len(s), -np.inf, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):                                    # a clamped tap repeats one of the window: the maximum is the same
            m = np.maximum(m, depth[np.clip(iy + dy, 0, H - 1), np.clip(ix + dx, 0, W - 1)])
    return ok & (s[:, 2].astype(np.float32) <= m + np.float32(min_gap))


def bake(pos, faces, lay, proj, depth, images, normals=None, cam_pos=None, power=1.0, min_gap=0.0, fill=(0.5, 0.5, 0.5),
         fallback=None):
    """-> (colors float32 [H_a, W_a, 3], n_seen int32 [H_a, W_a]); depth [n, H, W] float32: the depth maps of all views"""
    pos, faces = np.asarray(pos, dtype=F64), np.asarray(faces, dtype=np.int64)
    proj = np.asarray(proj, dtype=F64)[:, :3, :]
    n, H, W = images.shape[:3]
    own = owners(lay, len(faces))
    colors = np.empty(own.shape + (3,), dtype=np.float32)
    colors[:] = np.asarray(fill, dtype=np.float32)
    n_seen = np.where(own >= 0, 0, -1).astype(np.int32)
    in_range = ((faces >= 0) & (faces < len(pos))).all(1)
    jj, ii = np.nonzero((own >= 0) & in_range[np.clip(own, 0, None)])
    f = own[jj, ii]
    tri = faces[f]
    with np.errstate(all="ignore"):
        b = barycentrics(lay["uv"][f], ii.astype(F64), jj.astype(F64))
        p = np.stack([mix(b, pos[tri[:, 0], c], pos[tri[:, 1], c], pos[tri[:, 2], c]) for c in range(3)], -1)
        if normals is not None:
            nrm = np.asarray(normals, dtype=F64)
            n0, n1, n2 = nrm[tri[:, 0]], nrm[tri[:, 1]], nrm[tri[:, 2]]
            mixed = np.stack([mix(b, n0[:, c], n1[:, c], n2[:, c]) for c in range(3)], -1)
            ln = length(mixed)
            t = np.where(ln > 0, mix(b, length(n0), length(n1), length(n2)) / ln, 0.0)
            nv = mixed * t[:, None]
        S, C, cnt = np.zeros(len(f)), np.zeros((len(f), 3)), np.zeros(len(f), dtype=np.int32)
        for v in range(n):
            P = proj[v]
            q = [((P[r, 0] * p[:, 0] + P[r, 1] * p[:, 1]) + P[r, 2] * p[:, 2]) + P[r, 3] for r in range(3)]
            s = np.stack([q[0] / q[2], q[1] / q[2], q[2]], -1)
            vis = seen(s, depth[v], min_gap)
            idx, wts = taps(s[:, 0], s[:, 1], H, W)
            g = np.ones(len(f))
            if normals is not None:
                d = F64(cam_pos[v]) - p
                ld = length(d)
                dot = (nv[:, 0] * (d[:, 0] / ld) + nv[:, 1] * (d[:, 1] / ld)) + nv[:, 2] * (d[:, 2] / ld)
                g = np.power(np.abs(dot), F64(power))
            for c in range(3):
                tp = [images[v, y, x, c].astype(F64) for y, x in idx]
                if images.dtype == np.uint8:
                    tp = [x / F64(255.0) for x in tp]
                col = (wts[0] * tp[0] + wts[1] * tp[1]) + (wts[2] * tp[2] + wts[3] * tp[3])
                C[:, c] = np.where(vis, C[:, c] + g * col, C[:, c])
            S = np.where(vis, S + g, S)
            cnt += vis
        ok = (S > 0) & np.isfinite(S)
        out = np.where(ok[:, None], (C / S[:, None]).astype(np.float32), np.asarray(fill, dtype=np.float32)[None])
        if fallback is not None:
            fb = np.asarray(fallback, dtype=np.float32).astype(F64)
            fmix = np.stack([mix(b, fb[tri[:, 0], c], fb[tri[:, 1], c], fb[tri[:, 2], c]) for c in range(3)], -1)
            out = np.where(ok[:, None], out, fmix.astype(np.float32))
    colors[jj, ii] = out
    n_seen[jj, ii] = np.where(ok, cnt, 0)
    return colors, n_seen


def shade(face, bary, lay, texture, background=(0.0, 0.0, 0.0)):
    """face int32 [n, H, W], bary float32 [n, H, W, 3], texture float32 [H_a, W_a, 3] -> float32 [n, H, W, 3]"""
    out = np.empty(face.shape + (3,), dtype=np.float32)
    out[:] = np.asarray(background, dtype=np.float32)
    hit = (face >= 0) & (face < len(lay["uv"]))
    uv = lay["uv"][face[hit]]
    b = [bary[hit][:, k].astype(F64) for k in range(3)]
    with np.errstate(all="ignore"):
        u, w = mix(b, uv[:, 0, 0], uv[:, 1, 0], uv[:, 2, 0]), mix(b, uv[:, 0, 1], uv[:, 1, 1], uv[:, 2, 1])
        idx, wts = taps(u, w, lay["H"], lay["W"])
        cols = []
        for c in range(3):
            tp = [texture[y, x, c].astype(F64) for y, x in idx]
            cols.append(((wts[0] * tp[0] + wts[1] * tp[1]) + (wts[2] * tp[2] + wts[3] * tp[3])).astype(np.float32))
    out[hit] = np.stack(cols, -1)
    return out
