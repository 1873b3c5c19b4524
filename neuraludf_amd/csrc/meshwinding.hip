// The generalised winding number of a triangle mesh at query points (include/nudf.h NudfPointCloud, no new field):
// inside / outside that survives holes and open sheets; what libigl's fast_winding_number answers on the CPU.
//   wn_faces  -- one thread per face: the Morton key of the leaf cell of its centroid (-1 for an absent face); in point
//                mode one thread per query point: the key of its cell, for the driver's coherence sort;
//   wn_nodes  -- one thread per node of one level of the linear octree: raw moments about the grid's lower corner (a leaf
//                sums its faces in sorted order, a parent its children in preorder), shifted to the area-weighted centre;
//   winding   -- one wavefront walks the preorder for its 64 queries together: the node index is wave-uniform, every lane
//                carries the index at which it resumes, a far node adds its order-2 expansion, a near leaf its faces'
//                exact solid angles (van Oosterom-Strackee).  Per lane the walk is that of DESIGN.md 4.22 whatever the
//                other 63 lanes hold.
// No kernel uses atomics, LDS or scratch.  Float64 with no contraction: products and sums go through mul / add / sub of
// f64_exact.h, quotients and roots through the correctly rounded __ddiv_rn / __dsqrt_rn; only atan2 is not bit-defined.
// Restated in tests/meshwinding_ref.py.
#pragma clang fp contract(off)

#include "cell_index.h"
#include "mesh_launch.h"

#define WN_BLOCK 256
#define WN_RAW 40            // doubles per node of the raw moments: W, M[3], S[3], T0[9], Q0[18], lo[3], hi[3]
#define WN_REC 32            // doubles per node record: centre[3], r2, S[3], T diag[3], T off[3], Q[18], tr T
#define WN_FACES 0
#define WN_POINTS 1
#define WN_FOUR_PI 12.566370614359172

__device__ __forceinline__ double quo(double x, double y) { return __ddiv_rn(x, y); }

// ---- keys ---------------------------------------------------------------------------------------------------------------
// bit k of x goes to bit 3 k (21 bits)
__device__ __forceinline__ uint64_t spread3(uint64_t x) {
  x &= 0x1fffffULL;
  x = (x | (x << 32)) & 0x1f00000000ffffULL;
  x = (x | (x << 16)) & 0x1f0000ff0000ffULL;
  x = (x | (x << 8)) & 0x100f00f00f00f00fULL;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ULL;
  x = (x | (x << 2)) & 0x1249249249249249ULL;
  return x;
}

__device__ __forceinline__ int64_t morton(int64_t x, int64_t y, int64_t z) {
  return (int64_t)((spread3((uint64_t)x) << 2) | (spread3((uint64_t)y) << 1) | spread3((uint64_t)z));
}

__device__ __forceinline__ int64_t leaf_axis(const NudfPointCloud& a, double v, int x) {
  const int64_t c = cell_coord(v, a.origin[x], a.cell);
  return c < 0 ? 0 : (c >= a.grid[x] ? a.grid[x] - 1 : c);
}

// ---- a face ---------------------------------------------------------------------------------------------------------------
struct Tri {
  V3 a, b, c;
};

__device__ __forceinline__ bool finite3(const V3& v) { return is_finite(v.x) && is_finite(v.y) && is_finite(v.z); }

// false: an index out of range (nothing is read)
__device__ __forceinline__ bool load_corners(const NudfPointCloud& a, int64_t f, Tri& t) {
  const int64_t* fi = a.faces + 3 * f;
  const int64_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.n_verts || i1 >= a.n_verts || i2 >= a.n_verts) return false;
  t.a = vload(a.verts + 3 * i0), t.b = vload(a.verts + 3 * i1), t.c = vload(a.verts + 3 * i2);
  return true;
}

// the area vector 1/2 (b - a) x (c - a) and its length; false: the face is absent
__device__ __forceinline__ bool area_of(const Tri& t, V3& A, double& len) {
  if (!(finite3(t.a) && finite3(t.b) && finite3(t.c))) return false;
  const V3 n = vcross(vsub(t.b, t.a), vsub(t.c, t.a));
  A = {mul(0.5, n.x), mul(0.5, n.y), mul(0.5, n.z)};
  len = __dsqrt_rn(dot3(A.x, A.y, A.z));
  return positive_finite(len);
}

__device__ __forceinline__ V3 centroid(const Tri& t) {
  return {quo(add(t.a.x, add(t.b.x, t.c.x)), 3.0), quo(add(t.a.y, add(t.b.y, t.c.y)), 3.0),
          quo(add(t.a.z, add(t.b.z, t.c.z)), 3.0)};
}

__global__ __launch_bounds__(WN_BLOCK) void pc_wn_faces_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * WN_BLOCK + threadIdx.x;
  if (t >= a.n_query) return;
  V3 c;
  if (a.md_mode == WN_POINTS) {
    c = vload(a.query + 3 * t);
  } else {
    Tri f;
    V3 A;
    double len;
    if (!load_corners(a, t, f) || !area_of(f, A, len)) {
      a.keys[t] = -1;
      return;
    }
    c = centroid(f);
  }
  a.keys[t] = morton(leaf_axis(a, c.x, 0), leaf_axis(a, c.y, 1), leaf_axis(a, c.z, 2));
}

// ---- node moments -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ constexpr int sym(int j, int k) { return j * 3 - j * (j - 1) / 2 + (k - j); }     // j <= k

// adds face t (area vector A of length len) to the raw moments m
__device__ __forceinline__ void add_face(const NudfPointCloud& a, const Tri& t, const V3& Av, double len, double* m) {
  const V3 cf = centroid(t);
  const double x[3] = {sub(cf.x, a.origin[0]), sub(cf.y, a.origin[1]), sub(cf.z, a.origin[2])};
  const double A[3] = {Av.x, Av.y, Av.z};
  const V3 d0 = vsub(t.a, cf), d1 = vsub(t.b, cf), d2 = vsub(t.c, cf);
  const double e0[3] = {d0.x, d0.y, d0.z}, e1[3] = {d1.x, d1.y, d1.z}, e2[3] = {d2.x, d2.y, d2.z};
  m[0] = add(m[0], len);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    m[1 + j] = add(m[1 + j], mul(len, x[j]));
    m[4 + j] = add(m[4 + j], A[j]);
#pragma unroll
    for (int k = 0; k < 3; ++k) m[7 + 3 * j + k] = add(m[7 + 3 * j + k], mul(x[j], A[k]));
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int k = j; k < 3; ++k) {
      const double C = quo(add(mul(e0[j], e0[k]), add(mul(e1[j], e1[k]), mul(e2[j], e2[k]))), 12.0);
      const double xx = add(mul(x[j], x[k]), C);
#pragma unroll
      for (int i = 0; i < 3; ++i) m[16 + 6 * i + sym(j, k)] = add(m[16 + 6 * i + sym(j, k)], mul(A[i], xx));
    }
  }
  m[34] = fmin(m[34], fmin(fmin(t.a.x, t.b.x), t.c.x)), m[37] = fmax(m[37], fmax(fmax(t.a.x, t.b.x), t.c.x));
  m[35] = fmin(m[35], fmin(fmin(t.a.y, t.b.y), t.c.y)), m[38] = fmax(m[38], fmax(fmax(t.a.y, t.b.y), t.c.y));
  m[36] = fmin(m[36], fmin(fmin(t.a.z, t.b.z), t.c.z)), m[39] = fmax(m[39], fmax(fmax(t.a.z, t.b.z), t.c.z));
}

__global__ __launch_bounds__(WN_BLOCK) void pc_wn_nodes_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * WN_BLOCK + threadIdx.x;
  if (t >= a.n_query) return;
  const int64_t i = a.query_idx[t];
  if (i < 0 || i >= a.n) return;
  double m[WN_RAW];
#pragma unroll
  for (int k = 0; k < 34; ++k) m[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) m[34 + k] = __builtin_inf(), m[37 + k] = -__builtin_inf();
  int64_t sk = a.rank[i];
  if (sk <= i || sk > a.n) sk = i + 1;
  if (sk == i + 1) {                                  // a leaf: its faces in sorted order
    const int64_t b = a.cell_start[i], e = b + a.cell_count[i];
    if (b >= 0 && e >= b && e <= a.md_n_refs) {
      for (int64_t s = b; s < e; ++s) {
        const int64_t f = a.md_cell_face[s];
        Tri tri;
        V3 A;
        double len;
        if (f < 0 || f >= a.n_faces || !load_corners(a, f, tri) || !area_of(tri, A, len)) continue;
        add_face(a, tri, A, len, m);
      }
    }
  } else {                                            // its children (at most 8), written by the launch of the level below
    int64_t c = i + 1;
    for (int child = 0; child < 8 && c < sk; ++child) {
      const double* r = a.out + WN_RAW * c;
#pragma unroll
      for (int k = 0; k < 34; ++k) m[k] = add(m[k], r[k]);
#pragma unroll
      for (int k = 0; k < 3; ++k) m[34 + k] = fmin(m[34 + k], r[34 + k]), m[37 + k] = fmax(m[37 + k], r[37 + k]);
      const int64_t nc = a.rank[c];
      if (nc <= c) break;
      c = nc;
    }
  }
  double* raw = a.out + WN_RAW * i;
#pragma unroll
  for (int k = 0; k < WN_RAW; ++k) raw[k] = m[k];
  // the shift to the area-weighted centre: delta = x - s with s = M / W
  const double s[3] = {quo(m[1], m[0]), quo(m[2], m[0]), quo(m[3], m[0])};
  const double S[3] = {m[4], m[5], m[6]};
  double T[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int k = 0; k < 3; ++k) T[3 * j + k] = sub(m[7 + 3 * j + k], mul(s[j], S[k]));
  }
  double* rec = a.md_point + WN_REC * i;
  double r2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ck = add(a.origin[k], s[k]);
    const double ext = fmax(sub(ck, m[34 + k]), sub(m[37 + k], ck));
    rec[k] = ck;
    r2 = k == 0 ? mul(ext, ext) : add(r2, mul(ext, ext));
    rec[4 + k] = S[k];
    rec[7 + k] = T[4 * k];
  }
  rec[3] = r2;
  rec[10] = add(T[1], T[3]), rec[11] = add(T[2], T[6]), rec[12] = add(T[5], T[7]);
#pragma unroll
  for (int i3 = 0; i3 < 3; ++i3) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int k = j; k < 3; ++k) {
        const double q0 = m[16 + 6 * i3 + sym(j, k)];
        rec[13 + 6 * i3 + sym(j, k)] =
            sub(sub(sub(q0, mul(s[k], T[3 * j + i3])), mul(s[j], T[3 * k + i3])), mul(mul(s[j], s[k]), S[i3]));
      }
    }
  }
  rec[31] = add(add(T[0], T[4]), T[8]);
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// the order-2 expansion of the node record rec seen along r = centre - q, d2 = |r|^2
__device__ __forceinline__ double expansion(const double* rec, const V3& r, double d2) {
  const double d = __dsqrt_rn(d2);
  const double d3 = mul(d2, d), d5 = mul(d3, d2), d7 = mul(d5, d2);
  const double xx = mul(r.x, r.x), yy = mul(r.y, r.y), zz = mul(r.z, r.z);
  const double xy = mul(r.x, r.y), xz = mul(r.x, r.z), yz = mul(r.y, r.z);
  const double t0 = quo(add(add(mul(rec[4], r.x), mul(rec[5], r.y)), mul(rec[6], r.z)), d3);
  const double rTr = add(add(add(mul(rec[7], xx), mul(rec[8], yy)), mul(rec[9], zz)),
                         add(add(mul(rec[10], xy), mul(rec[11], xz)), mul(rec[12], yz)));
  const double t1 = sub(quo(rec[31], d3), quo(mul(3.0, rTr), d5));
  double g[3], H[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* Q = rec + 13 + 6 * i;
    g[i] = add(add(add(mul(Q[0], xx), mul(Q[3], yy)), mul(Q[5], zz)),
               mul(2.0, add(add(mul(Q[1], xy), mul(Q[2], xz)), mul(Q[4], yz))));
    H[i] = add(add(Q[0], Q[3]), Q[5]);
  }
  const double cubic = add(add(mul(r.x, g[0]), mul(r.y, g[1])), mul(r.z, g[2]));
  const double V0 = add(add(rec[13 + 0], rec[19 + 1]), rec[25 + 2]);
  const double V1 = add(add(rec[13 + 1], rec[19 + 3]), rec[25 + 4]);
  const double V2 = add(add(rec[13 + 2], rec[19 + 4]), rec[25 + 5]);
  const double lin = add(mul(2.0, add(add(mul(V0, r.x), mul(V1, r.y)), mul(V2, r.z))),
                         add(add(mul(H[0], r.x), mul(H[1], r.y)), mul(H[2], r.z)));
  const double t2 = mul(0.5, add(quo(mul(-3.0, lin), d5), quo(mul(15.0, cubic), d7)));
  return add(add(t0, t1), t2);
}

// the solid angle of face t seen from q (van Oosterom-Strackee); 0 when q lies in the face's plane
__device__ __forceinline__ double solid_angle(const Tri& t, const V3& q) {
  const V3 a = vsub(t.a, q), b = vsub(t.b, q), c = vsub(t.c, q);
  const double la = __dsqrt_rn(dot3(a.x, a.y, a.z)), lb = __dsqrt_rn(dot3(b.x, b.y, b.z)),
               lc = __dsqrt_rn(dot3(c.x, c.y, c.z));
  const double num = vdot(a, vcross(b, c));
  // symmetric in the last two corners: a face wound the other way gives the negated angle to the bit
  const double den = add(add(mul(la, mul(lb, lc)), mul(vdot(b, c), la)), add(mul(vdot(a, b), lc), mul(vdot(c, a), lb)));
  return num == 0.0 ? 0.0 : mul(2.0, atan2(num, den));
}

__global__ __launch_bounds__(WN_BLOCK) void pc_winding_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * WN_BLOCK + threadIdx.x;
  const bool active = t < a.n_query;
  const int n = (int)a.n;
  const V3 q = active ? vload(a.query + 3 * t) : V3{0.0, 0.0, 0.0};
  const double beta2 = a.r2;
  int resume = active ? 0 : n;                      // the first node this lane still has to look at
  double acc = 0.0;
  int64_t n_exact = 0, n_far = 0;
  int i = 0;
  // the wave moves forward by at least one node per step: at most n steps, whatever `rank` holds
  for (int step = 0; step < n && i < n; ++step) {
    i = __builtin_amdgcn_readfirstlane(i);
    const double* rec = a.pts + (int64_t)WN_REC * i;
    const int64_t sk64 = a.rank[i];
    const int sk = sk64 > i && sk64 <= n ? (int)sk64 : i + 1;
    const bool leaf = sk == i + 1;
    const bool part = i >= resume;
    const V3 r = vsub(vload(rec), q);
    const double d2 = dot3(r.x, r.y, r.z);
    const bool far = part && d2 > mul(beta2, rec[3]);
    if (far) {
      acc = add(acc, expansion(rec, r, d2));
      ++n_far;
      resume = sk;
    }
    const bool near_leaf = part && !far && leaf;
    if (__ballot(near_leaf) != 0) {
      const int64_t b = a.cell_start[i], e = b + a.cell_count[i];
      if (b >= 0 && e >= b && e <= a.md_n_refs) {
        for (int64_t s = b; s < e; ++s) {
          const int64_t f = a.md_cell_face[s];
          Tri tri;
          if (f < 0 || f >= a.n_faces || !load_corners(a, f, tri)) continue;
          if (near_leaf) {
            acc = add(acc, solid_angle(tri, q));
            ++n_exact;
          }
        }
      }
      if (near_leaf) resume = sk;
    }
    int next = i + 1;
    if (__ballot(part && !far && !leaf) == 0) {     // nobody descends: on to the first node that some lane waits for
      next = wave_min(resume);
      next = next > i ? next : i + 1;
    }
    i = next;
  }
  if (!active) return;
  const int64_t row = a.query_idx ? a.query_idx[t] : t;
  if (row < 0 || row >= a.n_query) return;
  a.dist[row] = quo(acc, WN_FOUR_PI);
  if (a.md_count) a.md_count[row] = n_exact;
  if (a.idx) a.idx[row] = n_far;
}

// ---- the launchers ----------------------------------------------------------------------------------------------------------
#define WN_2_31 (1LL << 31)

static const char* wn_check(const NudfPointCloud& a) {
  if (a.n_query >= WN_2_31 || a.n_faces >= WN_2_31 || a.n_verts >= WN_2_31 || a.n >= WN_2_31 || a.md_n_refs >= WN_2_31 ||
      a.n_faces < 0 || a.n_verts < 0 || a.n < 0 || a.md_n_refs < 0)
    return "n_query, n_faces, n_verts, n and md_n_refs must lie in [0, 2^31)";
  if (!(a.cell > 0.0) || !(a.cell < __builtin_inf())) return "cell must be a positive finite number";
  if (!grid_ok(a)) return "grid must lie in [1, 2^21] on every axis";
  if (!origin_ok(a)) return "origin must be finite";
  return nullptr;
}

extern "C" int nudf_pc_wn_faces(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_query <= 0) return 0;
  if (const char* why = wn_check(a)) return refuse("nudf_pc_wn_faces", why);
  if (a.md_mode != WN_FACES && a.md_mode != WN_POINTS)
    return refuse("nudf_pc_wn_faces", "unknown mode (md_mode must be 0 faces or 1 points)");
  if (a.md_mode == WN_FACES && a.n_query != a.n_faces) return refuse("nudf_pc_wn_faces", "face mode needs n_query == n_faces");
  if (!a.keys || (a.md_mode == WN_FACES ? !a.verts || !a.faces : !a.query)) return refuse("nudf_pc_wn_faces", "NULL buffer");
  MESH_LAUNCH(pc_wn_faces_kernel, a.n_query, WN_BLOCK, WN_BLOCK, "nudf_pc_wn_faces");
}

extern "C" int nudf_pc_wn_nodes(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_query <= 0) return 0;
  if (const char* why = wn_check(a)) return refuse("nudf_pc_wn_nodes", why);
  if (a.n <= 0 || a.md_n_refs <= 0 || a.n_faces <= 0) return refuse("nudf_pc_wn_nodes", "no nodes or no faces to sum");
  if (!a.verts || !a.faces || !a.md_cell_face || !a.rank || !a.cell_start || !a.cell_count || !a.query_idx || !a.out ||
      !a.md_point)
    return refuse("nudf_pc_wn_nodes", "NULL buffer");
  MESH_LAUNCH(pc_wn_nodes_kernel, a.n_query, WN_BLOCK, WN_BLOCK, "nudf_pc_wn_nodes");
}

extern "C" int nudf_pc_winding(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_query <= 0) return 0;
  if (const char* why = wn_check(a)) return refuse("nudf_pc_winding", why);
  if (!(a.r2 >= 1.0)) return refuse("nudf_pc_winding", "beta must be >= 1 (r2 holds beta * beta; inf: the exact sum)");
  if (a.n <= 0 || a.md_n_refs <= 0 || a.n_faces <= 0) return refuse("nudf_pc_winding", "no nodes or no faces to walk");
  if (!a.verts || !a.faces || !a.md_cell_face || !a.pts || !a.rank || !a.cell_start || !a.cell_count || !a.query || !a.dist)
    return refuse("nudf_pc_winding", "NULL buffer");
  MESH_LAUNCH(pc_winding_kernel, a.n_query, WN_BLOCK, WN_BLOCK, "nudf_pc_winding");
}
