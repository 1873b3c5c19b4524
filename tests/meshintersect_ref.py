"""Plain-Python float64 restatement of csrc/meshintersect.hip, operation by operation, one pair of
triangles at a time: the filtered orient3d / orient2d signs, the rule for two triangles without a shared vertex, the
shared-vertex rules of the self mode, and the broad phase (brute force over all pairs whose boxes overlap; `handed` walks
the cells as the kernel does).  Python floats are IEEE doubles and nothing here is contracted, so the GPU's pair set and
kinds must equal this bit for bit; tests/test_meshintersect_ref.py holds it to exact rational arithmetic."""
import numpy as np

NONE, CROSSING, COPLANAR, UNCERTAIN = 0, 1, 2, 3
KIND_NAMES = {CROSSING: "crossing", COPLANAR: "coplanar", UNCERTAIN: "uncertain"}
EPS = 2.0 ** -53
O3_BOUND = (7.0 + 56.0 * EPS) * EPS
O2_BOUND = (3.0 + 16.0 * EPS) * EPS
TINY = 2.0 ** -960
MESH_CELL_FACTOR = 3.0            # evaluation.MESH_CELL_FACTOR: the default cell of a MeshIndex


# ---- the filtered predicates -------------------------------------------------------------------------------------------
def certified(det, bound):
    if not bound > TINY:
        return 0
    return 1 if det > bound else (-1 if -det > bound else 0)


def o3(a, b, c, d):
    """the sign of det[a - d; b - d; c - d] in Shewchuk's order: +1 / -1 certified by the stage-A bound, 0 uncertain"""
    adx, bdx, cdx = a[0] - d[0], b[0] - d[0], c[0] - d[0]
    ady, bdy, cdy = a[1] - d[1], b[1] - d[1], c[1] - d[1]
    adz, bdz, cdz = a[2] - d[2], b[2] - d[2], c[2] - d[2]
    bdxcdy, cdxbdy = bdx * cdy, cdx * bdy
    cdxady, adxcdy = cdx * ady, adx * cdy
    adxbdy, bdxady = adx * bdy, bdx * ady
    det = (adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy)) + cdz * (adxbdy - bdxady)
    permanent = (((abs(bdxcdy) + abs(cdxbdy)) * abs(adz) + (abs(cdxady) + abs(adxcdy)) * abs(bdz))
                 + (abs(adxbdy) + abs(bdxady)) * abs(cdz))
    return certified(det, O3_BOUND * permanent)


def o2(a, b, c):
    detleft = (a[0] - c[0]) * (b[1] - c[1])
    detright = (a[1] - c[1]) * (b[0] - c[0])
    return certified(detleft - detright, O2_BOUND * (abs(detleft) + abs(detright)))


# ---- the coplanar branch -----------------------------------------------------------------------------------------------
def drop_axis(f):
    a, b, c = f
    u = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    v = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    k, am = 0, abs(n[0])
    if abs(n[1]) > am:
        k, am = 1, abs(n[1])
    if abs(n[2]) > am:
        k = 2
    return k


def flat(v, k):
    return (v[(k + 1) % 3], v[(k + 2) % 3])


def edge_separates(a, b, c, others):
    s = o2(a, b, c)
    if s == 0:
        return False
    return all(o2(a, b, p) == -s for p in others)


def outside(v, p, q, s, x):
    return o2(v, p, x) == -s or o2(v, x, q) == -s


def coplanar(f, g, shared):
    k = drop_axis(f)
    fa, fb, fc = (flat(v, k) for v in f)
    ga, gb, gc = (flat(v, k) for v in g)
    if shared:
        sep = (edge_separates(fa, fb, fc, (gb, gc)) or edge_separates(fc, fa, fb, (gb, gc))
               or edge_separates(ga, gb, gc, (fb, fc)) or edge_separates(gc, ga, gb, (fb, fc)))
        if not sep:
            sf, sg = o2(fa, fb, fc), o2(ga, gb, gc)
            sep = (sf != 0 and sg != 0 and outside(fa, fb, fc, sf, gb) and outside(fa, fb, fc, sf, gc)
                   and outside(ga, gb, gc, sg, fb) and outside(ga, gb, gc, sg, fc))
    else:
        F, G = (fa, fb, fc), (ga, gb, gc)
        sep = (edge_separates(fa, fb, fc, G) or edge_separates(fb, fc, fa, G) or edge_separates(fc, fa, fb, G)
               or edge_separates(ga, gb, gc, F) or edge_separates(gb, gc, ga, F) or edge_separates(gc, ga, gb, F))
    return NONE if sep else COPLANAR


MISS, HIT, UNSURE = 0, 1, 2


def segment(d, e, sd, se, t):
    """the segment d e against the closed triangle t: it misses when both ends are certified on one side of t's plane, and
    when the signs of its line against t's three edges are certified and mixed, wherever the ends lie"""
    if sd != 0 and sd == se:
        return MISS
    s = (o3(d, e, t[0], t[1]), o3(d, e, t[1], t[2]), o3(d, e, t[2], t[0]))
    if 0 in s:
        return UNSURE
    if not s[0] == s[1] == s[2]:
        return MISS
    return HIT if sd != 0 and se != 0 else UNSURE


def by_edges(f, g, sf, sg):
    """two triangles meet only where an edge of one touches the other: the six edges"""
    r = [segment(s[k], s[(k + 1) % 3], sign[k], sign[(k + 1) % 3], t)
         for s, t, sign in ((f, g, sf), (g, f, sg)) for k in range(3)]
    if HIT in r:
        return CROSSING
    return NONE if all(x == MISS for x in r) else UNCERTAIN


# ---- two triangles with no shared vertex ---------------------------------------------------------------------------------
def from_corner(t, k):
    return (t[k], t[(k + 1) % 3], t[(k + 2) % 3])


def lone_first(t, s):
    k = 0 if s[1] == s[2] else (1 if s[0] == s[2] else 2)
    return from_corner(t, k), s[k]


def classify(f, g):
    sf = [o3(g[0], g[1], g[2], p) for p in f]
    if sf[0] != 0 and sf[0] == sf[1] == sf[2]:
        return NONE
    sg = [o3(f[0], f[1], f[2], p) for p in g]
    if sg[0] != 0 and sg[0] == sg[1] == sg[2]:
        return NONE
    if all(sf) and all(sg):
        F, lone_f = lone_first(f, sf)
        G, lone_g = lone_first(g, sg)
        if lone_f < 0:
            G = (G[0], G[2], G[1])
        if lone_g < 0:
            F = (F[0], F[2], F[1])
        d1, d2 = o3(F[0], F[1], G[0], G[1]), o3(F[0], F[2], G[2], G[0])
        if d1 > 0 or d2 > 0:
            return NONE
        return CROSSING if d1 < 0 and d2 < 0 else UNCERTAIN
    if not any(sf) or not any(sg):
        return coplanar(f, g, False)
    return by_edges(f, g, sf, sg)


# ---- shared vertices (self mode) -------------------------------------------------------------------------------------------
def classify_edge(f, gc):
    """f = (a, b, c) shares the edge a b with a face whose opposite corner is gc"""
    if o3(f[0], f[1], f[2], gc) != 0:
        return NONE
    k = drop_axis(f)
    a, b = flat(f[0], k), flat(f[1], k)
    s1, s2 = o2(a, b, flat(f[2], k)), o2(a, b, flat(gc, k))
    if s1 == 0 or s2 == 0:
        return UNCERTAIN
    return COPLANAR if s1 == s2 else NONE


def classify_vertex(f, g):
    """f[0] and g[0] are one vertex"""
    gb, gc = o3(f[0], f[1], f[2], g[1]), o3(f[0], f[1], f[2], g[2])
    fb, fc = o3(g[0], g[1], g[2], f[1]), o3(g[0], g[1], g[2], f[2])
    x, y = segment(g[1], g[2], gb, gc, f), segment(f[1], f[2], fb, fc, g)
    if x == HIT or y == HIT:
        return CROSSING
    if x == MISS and y == MISS:
        return NONE
    if (gb == 0 and gc == 0) or (fb == 0 and fc == 0):
        return coplanar(f, g, True)
    return UNCERTAIN


def classify_self(f, g, fi, gi):
    fi, gi = [int(i) for i in fi], [int(i) for i in gi]
    if len(set(fi)) < 3 or len(set(gi)) < 3:
        return classify(f, g)
    m = [gi.index(i) if i in gi else -1 for i in fi]
    ns = sum(k >= 0 for k in m)
    if ns == 0:
        return classify(f, g)
    if ns == 3:
        return NONE
    if ns == 2:
        kf = m.index(-1)
        kg = 3 - sum(k for k in m if k >= 0)
        return classify_edge(from_corner(f, (kf + 1) % 3), g[kg])
    kf = [k >= 0 for k in m].index(True)
    return classify_vertex(from_corner(f, kf), from_corner(g, m[kf]))


# ---- the broad phase -----------------------------------------------------------------------------------------------------
def _tri(c):
    return tuple(tuple(float(x) for x in p) for p in c)


def usable_corners(verts, faces):
    """([F, 3, 3] corner coordinates, [F] usable): a face with an index out of range or a non-finite coordinate is absent"""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    corners = verts[np.where(ok[:, None], faces, 0)] if len(verts) else np.zeros((len(faces), 3, 3))
    ok &= np.isfinite(corners).all((1, 2))
    return corners, ok


def box_pairs(ca, oka, cb, okb, self_mode):
    """the pairs (t, g) whose closed boxes overlap, ascending: what the narrow phase is handed"""
    lo_a, hi_a, lo_b, hi_b = ca.min(1), ca.max(1), cb.min(1), cb.max(1)
    out = []
    for t in np.nonzero(oka)[0]:
        hit = okb & (lo_a[t] <= hi_b).all(1) & (lo_b <= hi_a[t]).all(1)
        if self_mode:
            hit[:t + 1] = False
        out.extend((int(t), int(g)) for g in np.nonzero(hit)[0])
    return out


def tested(verts, faces, other=None):
    """-> [(a, b, kind)] of every pair the narrow phase is handed, ascending, NONE included: self mode over (verts, faces),
    or with other=(verts_b, faces_b) face a of the first mesh against face b of the second"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ca, oka = usable_corners(verts, faces)
    if other is None:
        return [(t, g, classify_self(_tri(ca[t]), _tri(ca[g]), faces[t], faces[g]))
                for t, g in box_pairs(ca, oka, ca, oka, True)]
    cb, okb = usable_corners(*other)
    return [(t, g, classify(_tri(ca[t]), _tri(cb[g]))) for t, g in box_pairs(ca, oka, cb, okb, False)]


def pairs(verts, faces, other=None):
    """the reported pairs -> [(a, b, kind)] sorted by (a, b): what MeshIndex.intersections returns"""
    return [r for r in tested(verts, faces, other) if r[2] != NONE]


def default_cell(verts, faces):
    c, ok = usable_corners(verts, faces)
    c = c[ok]
    return MESH_CELL_FACTOR * float((c.max(1) - c.min(1)).max(1).mean())


def handed(verts, faces, cell):
    """the pairs the kernel's walk hands to the narrow phase in self mode on a grid of edge `cell` -> list with
    repetitions, were there any: each face binned into every cell its box touches, thread t walking the cells of its own
    box and taking a pair only in the cell of the lower corner of the two boxes' intersection"""
    c, ok = usable_corners(verts, faces)
    origin = c[ok].min((0, 1))
    ext = c[ok].max((0, 1)) - origin
    grid = np.maximum(np.floor(ext / cell).astype(np.int64) + 1, 1)

    def cells(x):
        return np.clip(np.floor((x - origin) / cell).astype(np.int64), 0, grid - 1)

    lo, hi = c.min(1), c.max(1)
    table = {}
    for f in np.nonzero(ok)[0]:
        l, h = cells(lo[f]), cells(hi[f])
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    table.setdefault((x, y, z), []).append(int(f))
    out = []
    for t in np.nonzero(ok)[0]:
        l, h = cells(lo[t]), cells(hi[t])
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    for g in table.get((x, y, z), ()):
                        if g <= t:
                            continue
                        m = np.maximum(lo[t], lo[g])
                        if (m > hi[t]).any() or (m > hi[g]).any():
                            continue
                        if tuple(cells(m)) == (x, y, z):
                            out.append((int(t), g))
    return out


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
SHIFT_DIRECTION = (0.5370861555295747, 0.2915274230636872, 0.7915368220043530)     # generic: no symmetry plane of the sphere


def random_triangles(n=300, edge=0.2, seed=0):
    """n triangles in the unit cube with edges of about `edge`, no shared vertex -> (verts [3 n, 3], faces [n, 3])"""
    rng = np.random.default_rng(seed)
    centre = rng.random((n, 1, 3))
    verts = (centre + (rng.random((n, 3, 3)) - 0.5) * edge).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def two_spheres(level=2, shift=0.3):
    """two icospheres of radius 1, the second shifted by `shift` along SHIFT_DIRECTION -> ((va, fa), (vb, fb))"""
    import meshray_ref
    v, f = meshray_ref.icosphere(level)
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    return (v, f), (v + shift * np.array(SHIFT_DIRECTION), f.copy())


def merged(a, b):
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1] + len(a[0])])
