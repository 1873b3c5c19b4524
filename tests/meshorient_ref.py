"""numpy restatement of the face orientation and the vertex normals (neuraludf_amd/meshclean.py orient_faces /
vertex_normals, csrc/meshorient.hip), written from the definitions: manifold edges from a dictionary of the undirected
edges, a breadth-first parity walk over them, the choice between the two complementary sets of flips, and the
angle-weighted normals as a plain loop in Python floats (float64, one rounding per operation).  Python loops over faces
and corners: keep the meshes of the tests modest.  A plain helper module, not a conftest."""
import math
from collections import defaultdict, deque

import numpy as np

LANES = 64          # the outward sum: lane l adds the component's faces l, l + 64, ... in order, then the lanes in order


def manifold_edges(faces):
    """-> [(face a, face b, same direction)] of the undirected edges with exactly two half-edges, of two different faces
    neither of which repeats a vertex, in the order of (min vertex, max vertex)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    users = defaultdict(list)
    for i, t in enumerate(f.tolist()):
        for k in range(3):
            u, v = t[k], t[(k + 1) % 3]
            users[(min(u, v), max(u, v))].append((i, u))            # half-edge 3 i + k starts at u
    out = []
    for key in sorted(users):
        hs = users[key]
        if len(hs) == 2 and hs[0][0] != hs[1][0] and not degenerate[hs[0][0]] and not degenerate[hs[1][0]]:
            out.append((hs[0][0], hs[1][0], hs[0][1] == hs[1][1]))
    return out


def incompatible_edges(faces, only_faces=None):
    """number of manifold edges whose two faces run along them in the same direction (`only_faces`: a bool mask, count the
    edges between two faces of it only)"""
    return sum(1 for a, b, same in manifold_edges(faces)
               if same and (only_faces is None or (only_faces[a] and only_faces[b])))


def _outward_term(p, t, origin):
    """N_f . (c_f - origin), N_f = (p1 - p0) x (p2 - p0), c_f = (p0 + (p1 + p2)) / 3, one rounding per operation"""
    p0, p1, p2 = ([float(x) for x in p[v]] for v in t)
    u = [p1[i] - p0[i] for i in range(3)]
    w = [p2[i] - p0[i] for i in range(3)]
    n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
    d = [(p0[i] + (p1[i] + p2[i])) / 3.0 - origin[i] for i in range(3)]
    return (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]


def orient(verts, faces, outward_from=None):
    """-> (faces', flipped [F] bool, labels [F] int64, orientable [F] bool): the contract of orient_faces"""
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = len(f)
    nbr = defaultdict(list)
    for a, b, same in manifold_edges(f):
        nbr[a].append((b, same))
        nbr[b].append((a, same))
    labels = np.full(n, -1, dtype=np.int64)
    parity = np.zeros(n, dtype=bool)
    orientable = np.ones(n, dtype=bool)
    flipped = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for start in range(n):                              # ascending: `start` is the smallest face of its component
            if labels[start] >= 0:
                continue
            labels[start] = start
            members, ok, queue = [start], True, deque([start])
            while queue:
                a = queue.popleft()
                for b, same in nbr[a]:
                    if labels[b] < 0:
                        labels[b], parity[b] = start, parity[a] ^ same
                        members.append(b)
                        queue.append(b)
                    elif parity[b] != (parity[a] ^ same):
                        ok = False
            members.sort()
            if not ok:
                orientable[members] = False
                continue
            k = int(parity[members].sum())
            complement = k > len(members) - k               # tie: the set that leaves `start` alone
            if outward_from is not None:
                origin = [float(x) for x in outward_from]
                lane = [0.0] * LANES
                for j, m in enumerate(members):
                    t = f[m].tolist()
                    if parity[m]:
                        t = [t[0], t[2], t[1]]
                    lane[j % LANES] = lane[j % LANES] + _outward_term(p, t, origin)
                s = 0.0
                for x in lane:
                    s = s + x
                if math.isfinite(s) and s != 0.0:
                    complement = s < 0.0
            flipped[members] = parity[members] ^ complement
    out = f.copy()
    out[flipped] = f[flipped][:, [0, 2, 1]]
    return out, flipped, labels, orientable


def signed_volume(verts, faces):
    p = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)


def vertex_normals(verts, faces, return_length=False):
    """angle-weighted vertex normals, float64 [V, 3]: at corner k of face f the weight is atan2(|n_f|, e1 . e2), the
    corners at a vertex summed in ascending 3 f + k.  return_length: also |N_v| [V], the length of the sum before it is
    normalised (a difference of d in one term moves the normal by about d / |N_v|)"""
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    acc = [[0.0, 0.0, 0.0] for _ in range(len(p))]
    with np.errstate(all="ignore"):
        for t in f.tolist():                                # ascending f, then k: ascending 3 f + k at every vertex
            q = [[float(x) for x in p[v]] for v in t]
            u = [q[1][i] - q[0][i] for i in range(3)]
            w = [q[2][i] - q[0][i] for i in range(3)]
            n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
            sq = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            ln = math.sqrt(sq) if sq >= 0.0 else float("nan")
            if not (ln > 0.0 and math.isfinite(ln)):
                continue
            unit = [float(np.float64(n[i]) / np.float64(ln)) for i in range(3)]
            for k in range(3):
                c, nx, pv = q[k], q[(k + 1) % 3], q[(k + 2) % 3]
                e1 = [nx[i] - c[i] for i in range(3)]
                e2 = [pv[i] - c[i] for i in range(3)]
                theta = math.atan2(ln, (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2])
                a = acc[t[k]]
                for i in range(3):
                    a[i] = a[i] + theta * unit[i]
        out = np.zeros((len(p), 3), dtype=np.float64)
        length = np.zeros(len(p), dtype=np.float64)
        for v, a in enumerate(acc):
            sq = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            ln = math.sqrt(sq) if sq >= 0.0 else float("nan")
            length[v] = ln
            if ln > 0.0 and math.isfinite(ln):
                out[v] = [float(np.float64(a[i]) / np.float64(ln)) for i in range(3)]
    return (out, length) if return_length else out


def vertex_normals_arccos(verts, faces):
    """trimesh's formula literally: the corner angle is the arccos of the dot product of the normalised edges, the face
    normals are normalised cross products, faces of zero area are left out"""
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = p[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    unit = n[ok] / ln[ok, None]
    tri, fo = tri[ok], f[ok]
    out = np.zeros_like(p)
    for k in range(3):
        e1 = tri[:, (k + 1) % 3] - tri[:, k]
        e2 = tri[:, (k + 2) % 3] - tri[:, k]
        e1 = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = e2 / np.linalg.norm(e2, axis=1, keepdims=True)
        theta = np.arccos(np.clip(np.einsum("ij,ij->i", e1, e2), -1.0, 1.0))
        np.add.at(out, fo[:, k], theta[:, None] * unit)
    ln = np.linalg.norm(out, axis=1)
    out[ln > 0] /= ln[ln > 0, None]
    return out


# ---- meshes of the tests ------------------------------------------------------------------------------------------------
def band(segments=12, twist=True, jitter=0.05, seed=7):
    """a band of `segments` quads round the z axis, vertices 2 i + j, quad i split as [a0, b0, b1], [a0, b1, a1]; the last
    quad closes onto (0, 1), (0, 0) with the twist (a Moebius band) and onto (0, 0), (0, 1) without it
    -> (verts float64 [2 segments, 3], faces int64 [2 segments, 3]).  The vertices are moved by a seeded +-jitter: the
    plain parametrisation is symmetric about the x axis, which puts the two faces at vertex 1 of the twisted band, wound
    against each other, into one plane with equal angles -- its normal would be the rounding error of a cancelled sum."""
    verts = np.zeros((2 * segments, 3))
    for i in range(segments):
        t = 2.0 * math.pi * i / segments
        for j, s in enumerate((-0.2, 0.2)):
            r = 1.0 + s * math.cos(t / 2.0) if twist else 1.0
            z = s * math.sin(t / 2.0) if twist else s
            verts[2 * i + j] = [r * math.cos(t), r * math.sin(t), z]
    verts += np.random.default_rng(seed).uniform(-jitter, jitter, verts.shape)
    faces = []
    for i in range(segments):
        a0, a1 = 2 * i, 2 * i + 1
        b0, b1 = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < segments else ((1, 0) if twist else (0, 1))
        faces += [[a0, b0, b1], [a0, b1, a1]]
    return verts, np.array(faces, dtype=np.int64)


def strip(n, seed=None):
    """a strip of n faces in which face i touches faces i - 1 and i + 1 only (the chain of the face_components test),
    wound consistently; with a seed the faces are numbered at random and a third of them flipped
    -> (verts float64 [n + 2, 3], faces int64 [n, 3])"""
    i = np.arange(n)
    f = np.stack([i, i + 1, i + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    verts = np.stack([(np.arange(n + 2) // 2).astype(np.float64), (np.arange(n + 2) % 2).astype(np.float64),
                      np.zeros(n + 2)], 1)
    if seed is not None:
        rng = np.random.default_rng(seed)
        f = f[rng.permutation(n)]
        flip = rng.random(n) < 1.0 / 3.0
        f[flip] = f[flip][:, [0, 2, 1]]
    return verts, f


def mixed_mesh(sphere, patch, seed=11):
    """one mesh out of a closed surface and an open patch ((verts, faces) each), the Moebius band, three faces on one
    edge, a face with a repeated vertex and two vertices no face uses; the faces in a seeded random order, a seeded third
    of them flipped -> (verts float64 [V, 3], faces int64 [F, 3])"""
    bv, bf = band(12, twist=True)
    fan_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0.5], [0.5, 0.5, 1]], dtype=np.float64)
    fan_f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 2, 4]])                # the last one repeats a vertex
    parts = [(np.asarray(sphere[0], dtype=np.float64), sphere[1]), (bv + [3.0, 0.0, 0.0], bf),
             (np.asarray(patch[0], dtype=np.float64) + [0.0, 0.0, 2.0], patch[1]), (fan_v + [5.0, 0.0, 0.0], fan_f)]
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(np.asarray(f, dtype=np.int64) + base)
        base += len(v)
    verts.append(np.array([[7.0, 7.0, 7.0], [-7.0, 7.0, 7.0]]))
    verts, faces = np.concatenate(verts), np.concatenate(faces)
    rng = np.random.default_rng(seed)
    faces = faces[rng.permutation(len(faces))]
    flip = rng.random(len(faces)) < 1.0 / 3.0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return verts, faces
