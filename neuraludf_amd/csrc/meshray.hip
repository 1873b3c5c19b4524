// Rays against a triangle mesh (include/nudf.h NudfPointCloud, the md_ray fields): what a caller otherwise leaves the GPU
// for, trimesh.ray's intersects_first / intersects_any / intersects_location and Trimesh.contains.
//   raycast -- one thread per ray (sorted by the cell in which it enters the grid): walks the ray through the hashed cell
//              table that MeshIndex built for meshdist.hip (every face listed in every cell its box touches) and applies
//              the per-(ray, face) rule to the faces of the cells it visits.  Three modes: the first hit (smallest
//              (t, face)), any hit (early exit), the number of faces crossed.
// The cell key, the hash and PC_CELL_MARGIN are those of cell_index.h, shared with pointcloud.hip and meshdist.hip, whose
// kernels build the table.
// The rule (restated in tests/meshray_ref.py) is float64 with no contraction: products and sums go through
// mul / add / sub of f64_exact.h, plain operators under the pragma; the only fused instructions left are inside the
// correctly rounded __ddiv_rn expansion.  The walk decides which faces are looked at, never what a face answers: it is
// conservative, so the result depends neither on the cell size nor on the order of traversal.
#pragma clang fp contract(off)

#include "cell_index.h"
#include "mesh_launch.h"

#define MR_BLOCK 256
#define MR_FIRST 0
#define MR_ANY 1
#define MR_COUNT 2

__device__ __forceinline__ double pick(const V3& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// ---- the per-(ray, face) rule ---------------------------------------------------------------------------------------------
struct Ray {
  V3 o, d;
  int kx, ky, kz;        // the permuted axes: kz the axis of the largest |d|, the lowest on a tie
  double Sx, Sy, Sz;     // d_x / d_z, d_y / d_z, 1 / d_z
  double t_min, t_max;
};

struct Hit {
  double t;
  double w[3];           // at the face's corner order
  bool inclusive;        // first / any: all three edge functions >= 0 or all three <= 0
  bool crossing;         // count: the signs agree, a zero counting as positive in the edge's own direction
};

struct P3 {
  double x, y, z;
};

__device__ __forceinline__ P3 shear(const Ray& r, const V3& v) {
  const V3 p = vsub(v, r.o);
  const double pz = pick(p, r.kz);
  return {sub(pick(p, r.kx), mul(r.Sx, pz)), sub(pick(p, r.ky), mul(r.Sy, pz)), mul(r.Sz, pz)};
}

__device__ __forceinline__ double edge(const P3& p, const P3& q) { return sub(mul(p.x, q.y), mul(p.y, q.x)); }

// false: the face is absent, or not hit in the ray's window under either reading
__device__ __forceinline__ bool ray_face(const NudfPointCloud& a, const Ray& r, int64_t f, Hit& h) {
  const int64_t* fi = a.faces + 3 * f;
  const int64_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.n_verts || i1 >= a.n_verts || i2 >= a.n_verts) return false;
  V3 A = vload(a.verts + 3 * i0), B = vload(a.verts + 3 * i1), C = vload(a.verts + 3 * i2);
  if (!(is_finite(A.x) && is_finite(A.y) && is_finite(A.z) && is_finite(B.x) && is_finite(B.y) && is_finite(B.z) &&
        is_finite(C.x) && is_finite(C.y) && is_finite(C.z)))
    return false;
  // the corners in ascending vertex index (A, B, C at corners ka, kb, kc), each edge function once, from the lower index
  // to the higher: the winding and the corner a face starts at change no bit, and two faces that share an edge read the
  // same number off it
  int64_t ia = i0, ib = i1, ic = i2;
  int ka = 0, kb = 1, kc = 2;
#define MR_ORDER(IX, IY, KX, KY, X, Y) \
  if (IX > IY) {                        \
    const int64_t ti = IX;              \
    IX = IY, IY = ti;                   \
    const int tk = KX;                  \
    KX = KY, KY = tk;                   \
    const V3 tv = X;                    \
    X = Y, Y = tv;                      \
  }
  MR_ORDER(ia, ib, ka, kb, A, B)
  MR_ORDER(ib, ic, kb, kc, B, C)
  MR_ORDER(ia, ib, ka, kb, A, B)
#undef MR_ORDER
  const P3 pa = shear(r, A), pb = shear(r, B), pc = shear(r, C);
  const double cBC = edge(pb, pc), cAC = edge(pa, pc), cAB = edge(pa, pb);
  const double wA = cBC, wB = -cAC, wC = cAB;
  const double det = add(add(wA, wB), wC);
  if (!(det != 0.0)) return false;
  const double t = __ddiv_rn(add(add(mul(wA, pa.z), mul(wB, pb.z)), mul(wC, pc.z)), det);
  if (!(t >= r.t_min && t <= r.t_max && t < __longlong_as_double(0x7ff0000000000000LL))) return false;
  h.inclusive = (wA >= 0.0 && wB >= 0.0 && wC >= 0.0) || (wA <= 0.0 && wB <= 0.0 && wC <= 0.0);
  const bool sA = cBC >= 0.0, sB = !(cAC >= 0.0), sC = cAB >= 0.0;
  h.crossing = sA == sB && sB == sC;
  if (!h.inclusive && !h.crossing) return false;
  h.t = t;
  const double ua = __ddiv_rn(wA, det), ub = __ddiv_rn(wB, det), uc = __ddiv_rn(wC, det);
  h.w[0] = ka == 0 ? ua : (kb == 0 ? ub : uc);
  h.w[1] = ka == 1 ? ua : (kb == 1 ? ub : uc);
  h.w[2] = ka == 2 ? ua : (kb == 2 ? ub : uc);
  return true;
}

// the cell that owns a crossing (count mode: a face is listed in several cells and counts once): the cell of the
// computed hit point, clamped into the face's own cell box -- a pure function of the ray, the face and the grid
__device__ __forceinline__ void owner_cell(const NudfPointCloud& a, const Ray& r, int64_t f, double t, int64_t c[3]) {
  const int64_t* fi = a.faces + 3 * f;
  const double p[3] = {add(r.o.x, mul(t, r.d.x)), add(r.o.y, mul(t, r.d.y)), add(r.o.z, mul(t, r.d.z))};
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    int64_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                      // meshdist.hip face_cells: the box the face was binned by
      int64_t v = cell_coord(a.verts[3 * fi[k] + x], a.origin[x], a.cell);
      v = v < 0 ? 0 : (v >= a.grid[x] ? a.grid[x] - 1 : v);
      lo = (k == 0 || v < lo) ? v : lo;
      hi = (k == 0 || v > hi) ? v : hi;
    }
    const int64_t q = cell_coord(p[x], a.origin[x], a.cell);
    c[x] = q < lo ? lo : (q > hi ? hi : q);
  }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
// first and last cell of a range of cell units [u0, u1] on an axis of g cells; an empty range has lo > hi.  A NaN gives
// the widest range: more cells looked at, never fewer, and always inside the grid.
__device__ __forceinline__ int64_t lo_cell(double u, int64_t g) {
  return u >= (double)g ? g : (u >= 0.0 ? (int64_t)floor(u) : 0);
}
__device__ __forceinline__ int64_t hi_cell(double u, int64_t g) {
  return u < 0.0 ? -1 : (u < (double)g ? (int64_t)floor(u) : g - 1);
}
__device__ __forceinline__ double along(double uo, double ud, double t) { return ud == 0.0 ? uo : add(uo, mul(t, ud)); }

__global__ __launch_bounds__(MR_BLOCK) void pc_raycast_kernel(NudfPointCloud a) {
  const int64_t i = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= a.n_query) return;
  const int64_t out = a.query_idx[i];
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int mode = a.md_mode;
  Ray r;
  r.o = vload(a.md_ray_o + 3 * i);
  r.d = vload(a.md_ray_d + 3 * i);
  r.t_min = a.md_ray_window ? a.md_ray_window[2 * i] : a.md_t_min;
  r.t_max = a.md_ray_window ? a.md_ray_window[2 * i + 1] : a.md_t_max;
  const double ax = fabs(r.d.x), ay = fabs(r.d.y), az = fabs(r.d.z);
  r.kz = 0;
  double am = ax;
  if (ay > am) r.kz = 1, am = ay;
  if (az > am) r.kz = 2, am = az;
  r.kx = r.kz == 2 ? 0 : r.kz + 1;
  r.ky = r.kx == 2 ? 0 : r.kx + 1;
  const double dz = pick(r.d, r.kz);
  r.Sx = __ddiv_rn(pick(r.d, r.kx), dz);
  r.Sy = __ddiv_rn(pick(r.d, r.ky), dz);
  r.Sz = __ddiv_rn(1.0, dz);

  double best_t = inf;
  int64_t best_f = -1, count = 0;
  double best_w[3] = {nan, nan, nan};
  bool found = false;

  if (am > 0.0 && am < inf && r.t_min <= r.t_max) {
    // the ray in cell units, axes permuted: u(t) = uo + t ud; the grid is [0, g] on every axis
    const double m = PC_CELL_MARGIN;
    const V3 org = {a.origin[0], a.origin[1], a.origin[2]};
    const double uo[3] = {__ddiv_rn(sub(pick(r.o, r.kx), pick(org, r.kx)), a.cell),
                          __ddiv_rn(sub(pick(r.o, r.ky), pick(org, r.ky)), a.cell),
                          __ddiv_rn(sub(pick(r.o, r.kz), pick(org, r.kz)), a.cell)};
    const double ud[3] = {__ddiv_rn(pick(r.d, r.kx), a.cell), __ddiv_rn(pick(r.d, r.ky), a.cell), __ddiv_rn(dz, a.cell)};
    const int64_t g[3] = {a.grid[r.kx], a.grid[r.ky], a.grid[r.kz]};
    const double eps_t = __ddiv_rn(m, fabs(ud[2]));            // the margin as a step of t along the dominant axis
    // the window, then the grid box, both widened by the margin
    double w0 = sub(r.t_min, eps_t), w1 = add(r.t_max, eps_t);
    bool reach = ud[2] != 0.0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      if (ud[x] == 0.0) {
        reach = reach && uo[x] >= -m && uo[x] <= add((double)g[x], m);
      } else {
        const double ta = __ddiv_rn(sub(-m, uo[x]), ud[x]), tb = __ddiv_rn(sub(add((double)g[x], m), uo[x]), ud[x]);
        w0 = fmax(w0, fmin(ta, tb));
        w1 = fmin(w1, fmax(ta, tb));
      }
    }
    if (reach && w0 <= w1) {
      const double za = along(uo[2], ud[2], w0), zb = along(uo[2], ud[2], w1);
      const int64_t l0 = lo_cell(sub(fmin(za, zb), m), g[2]), l1 = hi_cell(add(fmax(za, zb), m), g[2]);
      const bool up = ud[2] > 0.0;
      for (int64_t n = 0; n <= l1 - l0 && !found; ++n) {
        const int64_t L = up ? l0 + n : l1 - n;
        // the t interval of the layer, straight from its two planes (widened), cut to the window
        const double ta = __ddiv_rn(sub(sub((double)L, m), uo[2]), ud[2]);
        const double tb = __ddiv_rn(sub(add((double)(L + 1), m), uo[2]), ud[2]);
        const double tl = fmax(fmin(ta, tb), w0), th = fmin(fmax(ta, tb), w1);
        const double xa = along(uo[0], ud[0], tl), xb = along(uo[0], ud[0], th);
        const double ya = along(uo[1], ud[1], tl), yb = along(uo[1], ud[1], th);
        const int64_t x0 = lo_cell(sub(fmin(xa, xb), m), g[0]), x1 = hi_cell(add(fmax(xa, xb), m), g[0]);
        const int64_t y0 = lo_cell(sub(fmin(ya, yb), m), g[1]), y1 = hi_cell(add(fmax(ya, yb), m), g[1]);
        for (int64_t X = x0; X <= x1 && !found; ++X) {
          for (int64_t Y = y0; Y <= y1 && !found; ++Y) {
            // back to the grid's own axes: kx = kz + 1, ky = kz + 2 (mod 3)
            const int64_t c0 = r.kz == 0 ? L : (r.kz == 1 ? Y : X);
            const int64_t c1 = r.kz == 0 ? X : (r.kz == 1 ? L : Y);
            const int64_t c2 = r.kz == 0 ? Y : (r.kz == 1 ? X : L);
            const int64_t row = cell_row(a, pack_key(c0, c1, c2));
            if (row < 0) continue;
            const int64_t b = a.cell_start[row], e = b + a.cell_count[row];
            for (int64_t s = b; s < e; ++s) {
              const int64_t f = a.md_cell_face[s];
              if (f < 0 || f >= a.n_faces || (mode == MR_FIRST && f == best_f)) continue;
              Hit h;
              if (!ray_face(a, r, f, h)) continue;
              if (mode == MR_COUNT) {
                if (!h.crossing) continue;
                int64_t oc[3];
                owner_cell(a, r, f, h.t, oc);
                count += (oc[0] == c0 && oc[1] == c1 && oc[2] == c2) ? 1 : 0;
              } else if (h.inclusive) {
                if (mode == MR_ANY) {
                  found = true;
                  break;
                }
                if (h.t < best_t || (h.t == best_t && f < best_f)) {
                  best_t = h.t, best_f = f;
                  best_w[0] = h.w[0], best_w[1] = h.w[1], best_w[2] = h.w[2];
                }
              }
            }
          }
        }
        // a hit below the plane where the ray leaves this layer, by the margin, cannot be beaten by a later layer
        if (mode == MR_FIRST) {
          const double leave = up ? sub((double)(L + 1), m) : add((double)L, m);
          if (best_t < __ddiv_rn(sub(leave, uo[2]), ud[2])) break;
        }
      }
    }
  }
  if (mode == MR_FIRST) {
    a.dist[out] = best_t;
    a.idx[out] = best_f;
    double* wo = a.md_bary + 3 * out;
    wo[0] = best_w[0], wo[1] = best_w[1], wo[2] = best_w[2];
  } else {
    a.md_count[out] = mode == MR_ANY ? (found ? 1 : 0) : count;
  }
}

// ---- the launcher ---------------------------------------------------------------------------------------------------------
#define MR_2_31 (1LL << 31)

extern "C" int nudf_pc_raycast(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_raycast";
  if (a.n_query <= 0) return 0;
  if (a.n_query >= MR_2_31 || a.n_faces >= MR_2_31 || a.n_verts >= MR_2_31 || a.n_faces < 0 || a.n_verts < 0)
    return refuse(entry, "n_query, n_faces and n_verts must lie in [0, 2^31)");
  if (!(a.cell > 0.0) || !(a.cell < __builtin_inf())) return refuse(entry, "cell must be a positive finite number");
  if (!grid_ok(a)) return refuse(entry, "grid must lie in [1, 2^21] on every axis");
  if (!origin_ok(a)) return refuse(entry, "origin must be finite");
  if (a.md_mode != MR_FIRST && a.md_mode != MR_ANY && a.md_mode != MR_COUNT)
    return refuse(entry, "unknown mode (md_mode must be 0 first, 1 any or 2 count)");
  if (a.md_t_min != a.md_t_min) return refuse(entry, "t_min is NaN");
  if (!(a.md_t_max >= a.md_t_min)) return refuse(entry, "t_max must be >= t_min");
  if (a.hash_cap < 2 || (a.hash_cap & (a.hash_cap - 1)) || a.n_cells <= 0 || a.hash_cap < 2 * a.n_cells)
    return refuse(entry, "hash_cap must be a power of two >= 2 n_cells, n_cells > 0");
  if (a.md_n_refs <= 0 || a.n_faces <= 0) return refuse(entry, "no faces or no references to search");
  if (!a.verts || !a.faces || !a.md_ray_o || !a.md_ray_d || !a.query_idx || !a.cell_start || !a.cell_count ||
      !a.hash_key || !a.hash_row || !a.md_cell_face)
    return refuse(entry, "NULL buffer");
  if (a.md_mode == MR_FIRST ? (!a.dist || !a.idx || !a.md_bary) : !a.md_count)
    return refuse(entry, "NULL output buffer (first: dist, idx, md_bary; any, count: md_count)");
  MESH_LAUNCH(pc_raycast_kernel, a.n_query, MR_BLOCK, MR_BLOCK, entry);
}
