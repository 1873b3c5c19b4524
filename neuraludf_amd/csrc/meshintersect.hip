// Which faces of a mesh pass through each other, or through the faces of a second mesh (include/nudf.h NudfPointCloud, no
// new field): what a caller otherwise leaves the GPU for, MeshLab's "select self intersecting faces", libigl or pymeshfix.
//   isect_count -- one thread per query triangle t: the number of pairs (t, g) it reports;
//   isect_emit  -- one thread per query triangle t: its pairs (t, g, kind) at the caller's exclusive scan of the counts.
// Both run pairs_of(), so a pair counted is a pair emitted; neither uses atomics.
// Self mode (md_mode 0): the query triangles are the faces of the indexed mesh, only g > t is looked at, and faces that
// share vertices by index follow the shared-vertex rules.  Two-mesh mode (md_mode 1): the index holds mesh B, the
// triangles of mesh A arrive as corner coordinates in `query` [n_query, 3, 3], every B face in reach is a candidate.
// Broad phase: thread t walks the cells its box touches (the range of meshdist.hip's tribin_count), drops a candidate
// whose box does not overlap its own (closed, exact) and handles the pair only in the cell that holds the lower corner
// of the two boxes' intersection: each pair once, no de-duplication buffer, and the set of tested pairs does not depend
// on the cell size.  The cell key and the hash are those of cell_index.h.
// Narrow phase (restated in tests/meshintersect_ref.py): every decision is the sign of an orient3d or
// orient2d of input coordinates, evaluated in Shewchuk's operation order with his stage-A error bound; a sign is
// certified when |det| > bound and bound > 2^-960, anything else is uncertain.  Float64 with no contraction: products
// and sums go through mul / add / sub of f64_exact.h, plain operators under the pragma.
// The contract: a pair that is not reported is disjoint in exact arithmetic, apart from the shared vertices (the shared
// edge, where two are shared); a CROSSING pair shares a point in exact arithmetic (other than the shared vertex); COPLANAR
// and UNCERTAIN pairs touch, overlap in a plane or come closer than float64 can tell: never silently dropped.
#pragma clang fp contract(off)

#include "cell_index.h"
#include "mesh_launch.h"

#define MI_BLOCK 256
#define MI_SELF 0
#define MI_TWO 1
#define MI_NONE 0

struct Tri {
  V3 a, b, c;
};

__device__ __forceinline__ double pick(const V3& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// ---- the filtered predicates ------------------------------------------------------------------------------------------------
#define MI_EPS 0x1p-53
#define MI_O3_BOUND ((7.0 + 56.0 * MI_EPS) * MI_EPS)
#define MI_O2_BOUND ((3.0 + 16.0 * MI_EPS) * MI_EPS)
#define MI_TINY 0x1p-960

__device__ __forceinline__ int certified(double det, double bound) {
  if (!(bound > MI_TINY)) return 0;
  return det > bound ? 1 : (-det > bound ? -1 : 0);
}

// the sign of det[a - d; b - d; c - d]: +1 / -1 certified, 0 uncertain
__device__ int o3(const V3& a, const V3& b, const V3& c, const V3& d) {
  const double adx = sub(a.x, d.x), bdx = sub(b.x, d.x), cdx = sub(c.x, d.x);
  const double ady = sub(a.y, d.y), bdy = sub(b.y, d.y), cdy = sub(c.y, d.y);
  const double adz = sub(a.z, d.z), bdz = sub(b.z, d.z), cdz = sub(c.z, d.z);
  const double bdxcdy = mul(bdx, cdy), cdxbdy = mul(cdx, bdy);
  const double cdxady = mul(cdx, ady), adxcdy = mul(adx, cdy);
  const double adxbdy = mul(adx, bdy), bdxady = mul(bdx, ady);
  const double det = add(add(mul(adz, sub(bdxcdy, cdxbdy)), mul(bdz, sub(cdxady, adxcdy))), mul(cdz, sub(adxbdy, bdxady)));
  const double permanent = add(add(mul(add(fabs(bdxcdy), fabs(cdxbdy)), fabs(adz)),
                                   mul(add(fabs(cdxady), fabs(adxcdy)), fabs(bdz))),
                               mul(add(fabs(adxbdy), fabs(bdxady)), fabs(cdz)));
  return certified(det, mul(MI_O3_BOUND, permanent));
}

struct P2 {
  double x, y;
};

// the sign of det[a - c; b - c] in the plane
__device__ __forceinline__ int o2(const P2& a, const P2& b, const P2& c) {
  const double detleft = mul(sub(a.x, c.x), sub(b.y, c.y));
  const double detright = mul(sub(a.y, c.y), sub(b.x, c.x));
  return certified(sub(detleft, detright), mul(MI_O2_BOUND, add(fabs(detleft), fabs(detright))));
}

// ---- the coplanar branch ------------------------------------------------------------------------------------------------------
// the axis of the largest component of f's normal (the lowest on a tie): the projection drops it
__device__ __forceinline__ int drop_axis(const Tri& f) {
  const V3 n = vcross(vsub(f.b, f.a), vsub(f.c, f.a));
  const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
  int k = 0;
  double am = ax;
  if (ay > am) k = 1, am = ay;
  if (az > am) k = 2;
  return k;
}

__device__ __forceinline__ P2 flat(const V3& v, int k) {
  return {pick(v, k == 2 ? 0 : k + 1), pick(v, k == 0 ? 2 : k - 1)};
}

// the line through a and b has c certified on one side and p, q (and r) certified on the other
__device__ __forceinline__ bool edge_separates(const P2& a, const P2& b, const P2& c, const P2& p, const P2& q, const P2& r,
                                               bool three) {
  const int s = o2(a, b, c);
  if (s == 0) return false;
  if (o2(a, b, p) != -s || o2(a, b, q) != -s) return false;
  return !three || o2(a, b, r) == -s;
}

// x certified outside the closed cone of apex v between the rays to p and q (s: the certified sign of o2(v, p, q))
__device__ __forceinline__ bool outside(const P2& v, const P2& p, const P2& q, int s, const P2& x) {
  return o2(v, p, x) == -s || o2(v, x, q) == -s;
}

// both triangles projected along f's axis: a certified separating edge of either makes them disjoint.  `shared`: the
// first corners of f and g are one vertex, which alone is no overlap: only the edges through it can separate, and they
// are held against the two free corners of the other triangle.  In a flat regular grid two faces around a vertex lie
// opposite each other with their edges on common lines, where no edge separates strictly: there the two cones at the
// shared vertex decide, which meet in it alone when each of the four free corners lies outside the other's cone.
__device__ int coplanar(const Tri& f, const Tri& g, bool shared) {
  const int k = drop_axis(f);
  const P2 fa = flat(f.a, k), fb = flat(f.b, k), fc = flat(f.c, k);
  const P2 ga = flat(g.a, k), gb = flat(g.b, k), gc = flat(g.c, k);
  if (shared) {
    if (edge_separates(fa, fb, fc, gb, gc, gc, false) || edge_separates(fc, fa, fb, gb, gc, gc, false) ||
        edge_separates(ga, gb, gc, fb, fc, fc, false) || edge_separates(gc, ga, gb, fb, fc, fc, false))
      return MI_NONE;
    const int sf = o2(fa, fb, fc), sg = o2(ga, gb, gc);
    if (sf != 0 && sg != 0 && outside(fa, fb, fc, sf, gb) && outside(fa, fb, fc, sf, gc) && outside(ga, gb, gc, sg, fb) &&
        outside(ga, gb, gc, sg, fc))
      return MI_NONE;
    return NUDF_ISECT_COPLANAR;
  }
  if (edge_separates(fa, fb, fc, ga, gb, gc, true) || edge_separates(fb, fc, fa, ga, gb, gc, true) ||
      edge_separates(fc, fa, fb, ga, gb, gc, true) || edge_separates(ga, gb, gc, fa, fb, fc, true) ||
      edge_separates(gb, gc, ga, fa, fb, fc, true) || edge_separates(gc, ga, gb, fa, fb, fc, true))
    return MI_NONE;
  return NUDF_ISECT_COPLANAR;
}

// selects value by value: a triangle picked through a pointer would live in scratch memory
__device__ __forceinline__ V3 sel(bool c, const V3& a, const V3& b) { return {c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }
__device__ __forceinline__ V3 corner(const Tri& t, int k) { return sel(k == 0, t.a, sel(k == 1, t.b, t.c)); }
__device__ __forceinline__ Tri from_corner(const Tri& t, int k) {      // the cyclic shift that starts at corner k
  return {corner(t, k), corner(t, k == 2 ? 0 : k + 1), corner(t, k == 0 ? 2 : k - 1)};
}

#define MI_MISS 0
#define MI_HIT 1
#define MI_UNSURE 2
// the segment d e against the closed triangle t, d and e of signs sd and se against its plane.  It misses when both ends
// are certified on one side, and when the three signs of its line against t's edges are certified and mixed: the line
// then misses the triangle, wherever the ends lie -- an end in the plane of t but outside t is decided this way.
__device__ __forceinline__ int segment(const V3& d, const V3& e, int sd, int se, const Tri& t) {
  if (sd != 0 && sd == se) return MI_MISS;
  const int s0 = o3(d, e, t.a, t.b), s1 = o3(d, e, t.b, t.c), s2 = o3(d, e, t.c, t.a);
  if (s0 == 0 || s1 == 0 || s2 == 0) return MI_UNSURE;
  if (s0 != s1 || s1 != s2) return MI_MISS;
  return sd != 0 && se != 0 ? MI_HIT : MI_UNSURE;
}

// two triangles meet only where an edge of one touches the other: the six edges, one after the other (a loop, not six
// copies of the predicates).  sf / sg: the signs of f's corners against g's plane and of g's against f's.
__device__ int by_edges(const Tri& f, const Tri& g, int f0, int f1, int f2, int g0, int g1, int g2) {
  bool all_miss = true, hit = false;
#pragma unroll 1
  for (int i = 0; i < 6; ++i) {
    const bool first = i < 3;
    const int k = first ? i : i - 3, k1 = k == 2 ? 0 : k + 1;
    const Tri s = {sel(first, f.a, g.a), sel(first, f.b, g.b), sel(first, f.c, g.c)};
    const Tri t = {sel(first, g.a, f.a), sel(first, g.b, f.b), sel(first, g.c, f.c)};
    const int s0 = first ? f0 : g0, s1 = first ? f1 : g1, s2 = first ? f2 : g2;
    const int sd = k == 0 ? s0 : (k == 1 ? s1 : s2), se = k1 == 0 ? s0 : (k1 == 1 ? s1 : s2);
    const int r = segment(corner(s, k), corner(s, k1), sd, se, t);
    hit = hit || r == MI_HIT;
    all_miss = all_miss && r == MI_MISS;
  }
  if (hit) return NUDF_ISECT_CROSSING;
  return all_miss ? MI_NONE : NUDF_ISECT_UNCERTAIN;
}

// ---- two triangles with no shared vertex ------------------------------------------------------------------------------------
// t with the corner whose sign differs from the other two first (a cyclic shift); *lone = that sign
__device__ __forceinline__ Tri lone_first(const Tri& t, int s0, int s1, int s2, int* lone) {
  const int k = s1 == s2 ? 0 : (s0 == s2 ? 1 : 2);
  *lone = k == 0 ? s0 : (k == 1 ? s1 : s2);
  return from_corner(t, k);
}

__device__ int classify(const Tri& f, const Tri& g) {
  const int f0 = o3(g.a, g.b, g.c, f.a), f1 = o3(g.a, g.b, g.c, f.b), f2 = o3(g.a, g.b, g.c, f.c);
  if (f0 != 0 && f0 == f1 && f1 == f2) return MI_NONE;
  const int g0 = o3(f.a, f.b, f.c, g.a), g1 = o3(f.a, f.b, f.c, g.b), g2 = o3(f.a, f.b, f.c, g.c);
  if (g0 != 0 && g0 == g1 && g1 == g2) return MI_NONE;
  if (f0 != 0 && f1 != 0 && f2 != 0 && g0 != 0 && g1 != 0 && g2 != 0) {
    // Guigue-Devillers: each lone corner first and on the positive side of the other triangle
    int sf, sg;
    const Tri F = lone_first(f, f0, f1, f2, &sf), G = lone_first(g, g0, g1, g2, &sg);
    const V3 Gb = sel(sf < 0, G.c, G.b), Gc = sel(sf < 0, G.b, G.c);
    const V3 Fb = sel(sg < 0, F.c, F.b), Fc = sel(sg < 0, F.b, F.c);
    const int d1 = o3(F.a, Fb, G.a, Gb), d2 = o3(F.a, Fc, Gc, G.a);
    if (d1 > 0 || d2 > 0) return MI_NONE;
    return d1 < 0 && d2 < 0 ? NUDF_ISECT_CROSSING : NUDF_ISECT_UNCERTAIN;
  }
  if ((f0 == 0 && f1 == 0 && f2 == 0) || (g0 == 0 && g1 == 0 && g2 == 0)) return coplanar(f, g, false);
  return by_edges(f, g, f0, f1, f2, g0, g1, g2);      // some corner in the other's plane, as far as float64 can tell
}

// ---- shared vertices (self mode) ----------------------------------------------------------------------------------------------
// f = (a, b, c) and g share the edge a b; gc is g's corner opposite to it
__device__ int classify_edge(const Tri& f, const V3& gc) {
  if (o3(f.a, f.b, f.c, gc) != 0) return MI_NONE;
  const int k = drop_axis(f);
  const P2 a = flat(f.a, k), b = flat(f.b, k);
  const int s1 = o2(a, b, flat(f.c, k)), s2 = o2(a, b, flat(gc, k));
  if (s1 == 0 || s2 == 0) return NUDF_ISECT_UNCERTAIN;
  return s1 == s2 ? NUDF_ISECT_COPLANAR : MI_NONE;             // the same side: a fold
}

// f.a and g.a are one vertex
__device__ int classify_vertex(const Tri& f, const Tri& g) {
  const int gb = o3(f.a, f.b, f.c, g.b), gc = o3(f.a, f.b, f.c, g.c);
  const int fb = o3(g.a, g.b, g.c, f.b), fc = o3(g.a, g.b, g.c, f.c);
  const int x = segment(g.b, g.c, gb, gc, f), y = segment(f.b, f.c, fb, fc, g);
  if (x == MI_HIT || y == MI_HIT) return NUDF_ISECT_CROSSING;
  if (x == MI_MISS && y == MI_MISS) return MI_NONE;
  if ((gb == 0 && gc == 0) || (fb == 0 && fc == 0)) return coplanar(f, g, true);
  return NUDF_ISECT_UNCERTAIN;
}

__device__ int classify_self(const Tri& f, const Tri& g, const int64_t* fi, const int64_t* gi) {
  const int64_t i0 = fi[0], i1 = fi[1], i2 = fi[2], j0 = gi[0], j1 = gi[1], j2 = gi[2];
  // a face that names a vertex twice has no shared-vertex rule: the general test answers UNCERTAIN or COPLANAR at worst
  if (i0 == i1 || i1 == i2 || i0 == i2 || j0 == j1 || j1 == j2 || j0 == j2) return classify(f, g);
  const int m0 = i0 == j0 ? 0 : (i0 == j1 ? 1 : (i0 == j2 ? 2 : -1));      // the corner of g that corner k of f is
  const int m1 = i1 == j0 ? 0 : (i1 == j1 ? 1 : (i1 == j2 ? 2 : -1));
  const int m2 = i2 == j0 ? 0 : (i2 == j1 ? 1 : (i2 == j2 ? 2 : -1));
  const int ns = (m0 >= 0) + (m1 >= 0) + (m2 >= 0);
  if (ns == 0) return classify(f, g);
  if (ns == 3) return MI_NONE;
  if (ns == 2) {
    const int kf = m0 < 0 ? 0 : (m1 < 0 ? 1 : 2);                           // f's free corner, then g's: 0 + 1 + 2 = 3
    const int kg = 3 - (m0 < 0 ? 0 : m0) - (m1 < 0 ? 0 : m1) - (m2 < 0 ? 0 : m2);
    const Tri F = from_corner(f, kf == 2 ? 0 : kf + 1);                     // the free corner last
    return classify_edge(F, corner(g, kg));
  }
  const int kf = m0 >= 0 ? 0 : (m1 >= 0 ? 1 : 2);
  return classify_vertex(from_corner(f, kf), from_corner(g, kf == 0 ? m0 : (kf == 1 ? m1 : m2)));
}

// ---- the broad phase --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite3(const V3& v) { return is_finite(v.x) && is_finite(v.y) && is_finite(v.z); }

// false: the face is absent (an index out of range, a non-finite coordinate)
__device__ __forceinline__ bool load_face(const NudfPointCloud& a, int64_t f, Tri& t) {
  const int64_t* fi = a.faces + 3 * f;
  const int64_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.n_verts || i1 >= a.n_verts || i2 >= a.n_verts) return false;
  t.a = vload(a.verts + 3 * i0), t.b = vload(a.verts + 3 * i1), t.c = vload(a.verts + 3 * i2);
  return finite3(t.a) && finite3(t.b) && finite3(t.c);
}

__device__ __forceinline__ double min3(double x, double y, double z) { return fmin(fmin(x, y), z); }
__device__ __forceinline__ double max3(double x, double y, double z) { return fmax(fmax(x, y), z); }

__device__ __forceinline__ int64_t grid_cell(const NudfPointCloud& a, double v, int x) {
  const int64_t c = cell_coord(v, a.origin[x], a.cell);
  return c < 0 ? 0 : (c >= a.grid[x] ? a.grid[x] - 1 : c);
}

// the pairs of query triangle t, in the order of the walk (cells x outermost, ascending face inside a cell): counted
// when `emit` is false, written at rows [row, end) when it is true -> their number
__device__ __forceinline__ int64_t pairs_of(const NudfPointCloud& a, int64_t t, bool emit, int64_t row, int64_t end) {
  const bool self = a.md_mode == MI_SELF;
  Tri f;
  if (self) {
    if (!load_face(a, t, f)) return 0;
  } else {
    const double* q = a.query + 9 * t;
    f.a = vload(q), f.b = vload(q + 3), f.c = vload(q + 6);
    if (!(finite3(f.a) && finite3(f.b) && finite3(f.c))) return 0;
  }
  const V3 lo = {min3(f.a.x, f.b.x, f.c.x), min3(f.a.y, f.b.y, f.c.y), min3(f.a.z, f.b.z, f.c.z)};
  const V3 hi = {max3(f.a.x, f.b.x, f.c.x), max3(f.a.y, f.b.y, f.c.y), max3(f.a.z, f.b.z, f.c.z)};
  // a query triangle of another mesh may lie outside the box of the indexed one: nothing to meet there
  if (hi.x < a.box_lo[0] || hi.y < a.box_lo[1] || hi.z < a.box_lo[2] || lo.x > a.box_hi[0] || lo.y > a.box_hi[1] ||
      lo.z > a.box_hi[2])
    return 0;
  const int64_t x0 = grid_cell(a, lo.x, 0), x1 = grid_cell(a, hi.x, 0);
  const int64_t y0 = grid_cell(a, lo.y, 1), y1 = grid_cell(a, hi.y, 1);
  const int64_t z0 = grid_cell(a, lo.z, 2), z1 = grid_cell(a, hi.z, 2);
  int64_t n = 0;
  for (int64_t X = x0; X <= x1; ++X) {
    for (int64_t Y = y0; Y <= y1; ++Y) {
      for (int64_t Z = z0; Z <= z1; ++Z) {
        const int64_t r = cell_row(a, pack_key(X, Y, Z));
        if (r < 0 || r >= a.n_cells) continue;
        const int64_t b = a.cell_start[r], e = b + a.cell_count[r];
        if (b < 0 || e > a.md_n_refs) continue;
        for (int64_t s = b; s < e; ++s) {
          const int64_t gidx = a.md_cell_face[s];
          if (gidx < 0 || gidx >= a.n_faces || (self && gidx <= t)) continue;
          Tri g;
          if (!load_face(a, gidx, g)) continue;
          // the boxes overlap (closed, exact), and this cell holds the lower corner of their intersection
          const double mx = fmax(lo.x, min3(g.a.x, g.b.x, g.c.x)), my = fmax(lo.y, min3(g.a.y, g.b.y, g.c.y));
          const double mz = fmax(lo.z, min3(g.a.z, g.b.z, g.c.z));
          if (mx > hi.x || my > hi.y || mz > hi.z || mx > max3(g.a.x, g.b.x, g.c.x) || my > max3(g.a.y, g.b.y, g.c.y) ||
              mz > max3(g.a.z, g.b.z, g.c.z))
            continue;
          if (grid_cell(a, mx, 0) != X || grid_cell(a, my, 1) != Y || grid_cell(a, mz, 2) != Z) continue;
          const int kind = self ? classify_self(f, g, a.faces + 3 * t, a.faces + 3 * gidx) : classify(f, g);
          if (kind == MI_NONE) continue;
          if (emit && row + n < end) {
            a.md_ref_key[row + n] = t;
            a.md_ref_face[row + n] = gidx;
            a.state[row + n] = (uint8_t)kind;
          }
          ++n;
        }
      }
    }
  }
  return n;
}

__global__ __launch_bounds__(MI_BLOCK) void pc_isect_count_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * MI_BLOCK + threadIdx.x;
  if (t >= a.n_query) return;
  a.md_ref_n[t] = pairs_of(a, t, false, 0, 0);
}

__global__ __launch_bounds__(MI_BLOCK) void pc_isect_emit_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * MI_BLOCK + threadIdx.x;
  if (t >= a.n_query) return;
  const int64_t n = a.md_ref_n[t], row = a.md_ref_off[t];
  if (n <= 0 || row < 0 || row > a.cap - n) return;                   // cap: the rows of the pair buffers
  pairs_of(a, t, true, row, row + n);
}

// ---- the launchers ----------------------------------------------------------------------------------------------------------
#define MI_2_31 (1LL << 31)

static const char* isect_check(const NudfPointCloud& a, bool emit) {
  if (a.n_query >= MI_2_31 || a.n_faces >= MI_2_31 || a.n_verts >= MI_2_31 || a.n_faces < 0 || a.n_verts < 0)
    return "n_query, n_faces and n_verts must lie in [0, 2^31)";
  if (!(a.cell > 0.0) || !(a.cell < __builtin_inf())) return "cell must be a positive finite number";
  if (!grid_ok(a)) return "grid must lie in [1, 2^21] on every axis";
  if (!origin_ok(a)) return "origin must be finite";
  if (a.md_mode != MI_SELF && a.md_mode != MI_TWO) return "unknown mode (md_mode must be 0 self or 1 two meshes)";
  if (a.md_mode == MI_SELF && a.n_query != a.n_faces) return "self mode needs n_query == n_faces";
  if (a.cap < 0) return "cap must not be negative";
  if (a.hash_cap < 2 || (a.hash_cap & (a.hash_cap - 1)) || a.n_cells <= 0 || a.hash_cap < 2 * a.n_cells)
    return "hash_cap must be a power of two >= 2 n_cells, n_cells > 0";
  if (a.md_n_refs <= 0 || a.n_faces <= 0) return "no faces or no references to search";
  if (!a.verts || !a.faces || !a.cell_start || !a.cell_count || !a.hash_key || !a.hash_row || !a.md_cell_face ||
      !a.md_ref_n || (a.md_mode == MI_TWO && !a.query))
    return "NULL buffer";
  if (emit && (!a.md_ref_off || !a.md_ref_key || !a.md_ref_face || !a.state))
    return "NULL output buffer (md_ref_off, md_ref_key, md_ref_face, state)";
  return nullptr;
}

extern "C" int nudf_pc_isect_count(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_query <= 0) return 0;
  if (const char* why = isect_check(a, false)) return refuse("nudf_pc_isect_count", why);
  MESH_LAUNCH(pc_isect_count_kernel, a.n_query, MI_BLOCK, MI_BLOCK, "nudf_pc_isect_count");
}

extern "C" int nudf_pc_isect_emit(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_query <= 0 || a.cap == 0) return 0;
  if (const char* why = isect_check(a, true)) return refuse("nudf_pc_isect_emit", why);
  MESH_LAUNCH(pc_isect_emit_kernel, a.n_query, MI_BLOCK, MI_BLOCK, "nudf_pc_isect_emit");
}
