"""A numpy float64 restatement of the rasteriser's six steps (include/nudf.h NudfMeshRaster, csrc/meshraster.hip): the
same expressions in the same order, with plain loops over views, faces, pixels and vertices.  Imported by the tests
only.  numpy multiplies, adds and divides float64 scalars one correctly rounded operation at a time, which is what the
kernels do with contraction off."""
import numpy as np

F64 = np.float64
EMPTY = (1 << 64) - 1


def camera_positions(proj):
    """-M^-1 p4 per view, float64"""
    return np.stack([-np.linalg.inv(P[:, :3]) @ P[:, 3] for P in np.asarray(proj, dtype=F64)[:, :3, :]])


def project(pos, proj):
    """-> scr [n_views, V, 3]: (q.x / q.z, q.y / q.z, q.z), each row of q as ((P0 x + P1 y) + P2 z) + P3"""
    pos, proj = np.asarray(pos, dtype=F64), np.asarray(proj, dtype=F64)[:, :3, :]
    scr = np.zeros((len(proj), len(pos), 3))
    with np.errstate(all="ignore"):
        for i, P in enumerate(proj):
            for v, (x, y, z) in enumerate(pos):
                q = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
                scr[i, v] = (q[0] / q[2], q[1] / q[2], q[2])
    return scr


def valid(s):
    return bool(np.isfinite(s[0]) and np.isfinite(s[1]) and np.isfinite(s[2]) and s[2] > 0)


def face_box(scr_view, tri, n_verts, H, W):
    """the face in one view -> None when it draws nothing, else (the nine screen values, xmin, ymin, bw, bh)"""
    v0, v1, v2 = (int(k) for k in tri)
    if min(v0, v1, v2) < 0 or max(v0, v1, v2) >= n_verts:
        return None
    if v0 == v1 or v1 == v2 or v0 == v2:
        return None
    s0, s1, s2 = scr_view[v0], scr_view[v1], scr_view[v2]
    if not (valid(s0) and valid(s1) and valid(s2)):
        return None
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = s0, s1, s2
    with np.errstate(all="ignore"):
        area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if not np.isfinite(area) or area == 0:
        return None
    xlo = max(np.ceil(min(x0, x1, x2)), 0.0)
    xhi = min(np.floor(max(x0, x1, x2)), float(W - 1))
    ylo = max(np.ceil(min(y0, y1, y2)), 0.0)
    yhi = min(np.floor(max(y0, y1, y2)), float(H - 1))
    if xlo > xhi or ylo > yhi:
        return None
    return (x0, y0, z0, x1, y1, z1, x2, y2, z2), int(xlo), int(ylo), int(xhi) - int(xlo) + 1, int(yhi) - int(ylo) + 1


def pixel(t, px, py):
    """the per-pixel function -> None when (px, py) is not covered, else ((b0, b1, b2), z)"""
    x0, y0, z0, x1, y1, z1, x2, y2, z2 = t
    x, y = F64(px), F64(py)
    with np.errstate(all="ignore"):
        ax, ay = x0 - x, y0 - y
        bx, by = x1 - x, y1 - y
        cx, cy = x2 - x, y2 - y
        w0 = bx * cy - cx * by
        w1 = cx * ay - ax * cy
        w2 = ax * by - bx * ay
        if not ((w0 >= 0 and w1 >= 0 and w2 >= 0) or (w0 <= 0 and w1 <= 0 and w2 <= 0)):
            return None
        s = (w0 + w1) + w2
        if not np.isfinite(s) or s == 0:
            return None
        b = (w0 / s, w1 / s, w2 / s)
        z = F64(1.0) / ((b[0] / z0 + b[1] / z1) + b[2] / z2)
    return b, z


def rasterize(pos, faces, proj, H, W, info=None):
    """-> (depth float32 [n, H, W], face int32 [n, H, W], bary float32 [n, H, W, 3]); info receives `skipped` (faces with
    an invalid vertex, summed over the views), `npix` [n, F] and `scr`"""
    pos, faces = np.asarray(pos, dtype=F64), np.asarray(faces, dtype=np.int64)
    scr = project(pos, proj)
    n, n_verts = len(scr), len(pos)
    zbuf = np.full((n, H, W), EMPTY, dtype=np.uint64)
    npix = np.zeros((n, len(faces)), dtype=np.int32)
    skipped = 0
    for i in range(n):
        for f, tri in enumerate(faces):
            if 0 <= min(tri) and max(tri) < n_verts and not all(valid(scr[i, k]) for k in tri):
                skipped += 1
            box = face_box(scr[i], tri, n_verts, H, W)
            if box is None:
                continue
            t, xmin, ymin, bw, bh = box
            npix[i, f] = bw * bh
            for j in range(bw * bh):                                  # row-major in the box
                px, py = xmin + j % bw, ymin + j // bw
                hit = pixel(t, px, py)
                if hit is None:
                    continue
                key = (int(np.float32(hit[1]).view(np.uint32)) << 32) | f
                if key < int(zbuf[i, py, px]):
                    zbuf[i, py, px] = key
    depth = np.full((n, H, W), np.inf, dtype=np.float32)
    face = np.full((n, H, W), -1, dtype=np.int32)
    bary = np.zeros((n, H, W, 3), dtype=np.float32)
    for i in range(n):
        for py in range(H):
            for px in range(W):
                key = int(zbuf[i, py, px])
                if key == EMPTY:
                    continue
                f = key & 0xffffffff
                depth[i, py, px] = np.uint32(key >> 32).view(np.float32)
                face[i, py, px] = f
                t = face_box(scr[i], faces[f], n_verts, H, W)[0]
                bary[i, py, px] = np.asarray(pixel(t, px, py)[0], dtype=np.float32)
    if info is not None:
        info.update(skipped=skipped, npix=npix, scr=scr)
    return depth, face, bary


def visible(scr, depth, min_gap):
    """-> vis uint8 [n, V]"""
    n, n_verts = scr.shape[:2]
    H, W = depth.shape[1:]
    gap = np.float32(min_gap)
    vis = np.zeros((n, n_verts), dtype=np.uint8)
    for i in range(n):
        for v in range(n_verts):
            s = scr[i, v]
            if not valid(s) or not (abs(s[0]) < 2.0 ** 52 and abs(s[1]) < 2.0 ** 52):
                continue
            px, py = np.rint(s[0]), np.rint(s[1])                     # half to even
            if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
                continue
            ix, iy = int(px), int(py)
            m = depth[i, max(iy - 1, 0):min(iy + 1, H - 1) + 1, max(ix - 1, 0):min(ix + 1, W - 1) + 1].max()
            vis[i, v] = np.float32(s[2]) <= np.float32(m) + gap
    return vis


def colour(pos, proj, vis, images, normals=None, cam_pos=None, power=1.0, fill=(0.5, 0.5, 0.5)):
    """-> (colors float32 [V, 3], n_seen int32 [V])"""
    pos = np.asarray(pos, dtype=F64)
    n, H, W = images.shape[:3]
    scr = project(pos, proj)
    colors = np.zeros((len(pos), 3), dtype=np.float32)
    n_seen = np.zeros(len(pos), dtype=np.int32)
    one = F64(1.0)
    with np.errstate(all="ignore"):
        for v, p in enumerate(pos):
            sw, sc, cnt = F64(0.0), [F64(0.0)] * 3, 0
            for i in range(n):
                if not vis[i, v]:
                    continue
                u, w = scr[i, v, 0], scr[i, v, 1]
                fx0, fy0 = np.floor(u), np.floor(w)
                fx, fy = u - fx0, w - fy0
                xa, xb = int(min(max(fx0, 0.0), W - 1)), int(min(max(fx0 + 1, 0.0), W - 1))
                ya, yb = int(min(max(fy0, 0.0), H - 1)), int(min(max(fy0 + 1, 0.0), H - 1))
                gx, gy = one - fx, one - fy
                w00, w10, w01, w11 = gx * gy, fx * gy, gx * fy, fx * fy
                g = one
                if normals is not None:
                    dx, dy, dz = (F64(cam_pos[i][k]) - p[k] for k in range(3))
                    length = np.sqrt((dx * dx + dy * dy) + dz * dz)
                    nv = np.asarray(normals[v], dtype=F64)
                    dot = (nv[0] * (dx / length) + nv[1] * (dy / length)) + nv[2] * (dz / length)
                    g = np.power(abs(dot), F64(power))

                def tap(y, x, c):
                    t = F64(images[i, y, x, c])
                    return t / F64(255.0) if images.dtype == np.uint8 else t

                for c in range(3):
                    col = (w00 * tap(ya, xa, c) + w10 * tap(ya, xb, c)) + (w01 * tap(yb, xa, c) + w11 * tap(yb, xb, c))
                    sc[c] = sc[c] + g * col
                sw = sw + g
                cnt += 1
            if sw > 0 and np.isfinite(sw):
                colors[v] = [np.float32(sc[c] / sw) for c in range(3)]
                n_seen[v] = cnt
            else:
                colors[v] = np.asarray(fill, dtype=np.float32)
    return colors, n_seen
