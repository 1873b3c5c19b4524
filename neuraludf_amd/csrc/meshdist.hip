// Exact point-to-mesh distance (include/nudf.h NudfPointCloud, the md_ fields): what a caller otherwise leaves the GPU for,
// trimesh.proximity.closest_point, or approximates with a KD-tree over surface samples.
//   tribin_count -- one thread per face: the number of cells its axis-aligned bounding box touches (0 for a face with an
//                   index out of range or a non-finite coordinate; cap + 1 when more than cap);
//   tribin_emit  -- one thread per face: (packed cell key, face) for each of those cells, at the caller's exclusive scan
//                   of the counts.  The caller sorts by key and builds the cell table and its hash with nudf_pc_cells;
//   closest      -- one thread per query (cell-sorted): the closest point of the mesh by Chebyshev rings of cells, up to
//                   `bound`: distance, face, point and barycentric weights.
// The cell key, the hash and the ring walk with its stop tests are those of cell_index.h, shared with pointcloud.hip,
// whose kernels build the table.  The ring stop holds for faces as it does for points: a face is listed in every cell
// its box touches, so a face not met in the rings <= k has its whole box, and with it every one of its points, outside
// the cube of those rings.
// The per-face rule (restated in tests/meshdist_ref.py) is float64 with no contraction: products and sums
// go through mul / add / sub of f64_exact.h, plain operators under the pragma; the only fused instructions left are
// inside the correctly rounded __ddiv_rn / __dsqrt_rn expansions (tests/test_meshdist_asm.py).
#pragma clang fp contract(off)

#include "cell_index.h"
#include "mesh_launch.h"

#define MD_BLOCK 256
#define MD_MAX_CAP (1LL << 40)          // largest reference count a caller may accept: F cap stays below 2^63

// ---- binning: a face goes into every cell its box touches ------------------------------------------------------------------
struct CellBox {
  int64_t lo[3], hi[3];
};

// false: a face that is absent (an index out of range, a NaN or infinite coordinate)
__device__ bool face_cells(const NudfPointCloud& a, int64_t f, CellBox& b) {
  const int64_t* fi = a.faces + 3 * f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (fi[k] < 0 || fi[k] >= a.n_verts) return false;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    int64_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = a.verts[3 * fi[k] + x];
      if (!is_finite(v)) return false;
      int64_t c = cell_coord(v, a.origin[x], a.cell);
      c = c < 0 ? 0 : (c >= a.grid[x] ? a.grid[x] - 1 : c);          // the grid holds every usable vertex: a safety net
      lo = (k == 0 || c < lo) ? c : lo;
      hi = (k == 0 || c > hi) ? c : hi;
    }
    b.lo[x] = lo;
    b.hi[x] = hi;
  }
  return true;
}

__global__ __launch_bounds__(MD_BLOCK) void pc_tribin_count_kernel(NudfPointCloud a) {
  const int64_t f = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  CellBox b;
  int64_t n = 0;
  if (face_cells(a, f, b)) {
    n = 1;
#pragma unroll
    for (int x = 0; x < 3; ++x) {                                      // each factor <= 2^21, n <= cap + 1 <= 2^40 + 1
      n *= b.hi[x] - b.lo[x] + 1;
      n = n > a.cap ? a.cap + 1 : n;
    }
  }
  a.md_ref_n[f] = n;
}

__global__ __launch_bounds__(MD_BLOCK) void pc_tribin_emit_kernel(NudfPointCloud a) {
  const int64_t f = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  const int64_t n = a.md_ref_n[f];
  if (n <= 0 || n > a.cap) return;
  CellBox b;
  if (!face_cells(a, f, b)) return;
  int64_t row = a.md_ref_off[f];
  const int64_t end = row + n;
  if (row < 0 || end > a.md_n_refs) return;
  for (int64_t x = b.lo[0]; x <= b.hi[0]; ++x)
    for (int64_t y = b.lo[1]; y <= b.hi[1]; ++y)
      for (int64_t z = b.lo[2]; z <= b.hi[2] && row < end; ++z, ++row) {
        a.md_ref_key[row] = pack_key(x, y, z);
        a.md_ref_face[row] = f;
      }
}

// ---- the per-face rule ---------------------------------------------------------------------------------------------------
struct Cand {
  double d2;
  V3 c;
  double w[3];     // at the face's corner order
};

// the segment from a (the lower vertex index, corner ka) to b (corner kb); replaces `best` when strictly closer
__device__ __forceinline__ void edge_candidate(const V3& p, const V3& a, const V3& b, int ka, int kb, Cand& best) {
  const V3 e = vsub(b, a);
  const double ee = dot3(e.x, e.y, e.z);
  const double t = ee == 0.0 ? 0.0 : __ddiv_rn(vdot(vsub(p, a), e), ee);
  V3 c;
  double wa, wb;
  if (t <= 0.0) {
    c = a, wa = 1.0, wb = 0.0;
  } else if (t >= 1.0) {
    c = b, wa = 0.0, wb = 1.0;
  } else {
    c = {add(a.x, mul(t, e.x)), add(a.y, mul(t, e.y)), add(a.z, mul(t, e.z))};
    wa = sub(1.0, t), wb = t;
  }
  const V3 r = vsub(p, c);
  const double d2 = dot3(r.x, r.y, r.z);
  if (d2 < best.d2) {
    best.d2 = d2;
    best.c = c;
    best.w[0] = best.w[1] = best.w[2] = 0.0;
    best.w[ka] = wa;
    best.w[kb] = wb;
  }
}

// the face's candidate: the interior one first, then the edges (i0,i1), (i1,i2), (i2,i0), the smallest d2, the earlier on
// a tie.  d2 = +inf when the face is absent.
__device__ __forceinline__ Cand face_candidate(const NudfPointCloud& a, int64_t f, const V3& p) {
  Cand best;
  best.d2 = __longlong_as_double(0x7ff0000000000000LL);
  best.c = {best.d2, best.d2, best.d2};
  best.w[0] = best.w[1] = best.w[2] = 0.0;
  const int64_t* fi = a.faces + 3 * f;
  const int64_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.n_verts || i1 >= a.n_verts || i2 >= a.n_verts) return best;
  const V3 v0 = vload(a.verts + 3 * i0), v1 = vload(a.verts + 3 * i1), v2 = vload(a.verts + 3 * i2);
  // the interior candidate is evaluated on the corners in ascending vertex index (A, B, C at corners ka, kb, kc), as
  // the edges are: the winding and the corner a face starts at change no bit of it.  (Equal indices: n = 0 exactly.)
  V3 A = v0, B = v1, C = v2;
  int64_t ia = i0, ib = i1, ic = i2;
  int ka = 0, kb = 1, kc = 2;
#define MD_ORDER(IX, IY, KX, KY, X, Y) \
  if (IX > IY) {                        \
    const int64_t ti = IX;              \
    IX = IY, IY = ti;                   \
    const int tk = KX;                  \
    KX = KY, KY = tk;                   \
    const V3 tv = X;                    \
    X = Y, Y = tv;                      \
  }
  MD_ORDER(ia, ib, ka, kb, A, B)
  MD_ORDER(ib, ic, kb, kc, B, C)
  MD_ORDER(ia, ib, ka, kb, A, B)
#undef MD_ORDER
  const V3 n = vcross(vsub(B, A), vsub(C, A));
  const double nn = dot3(n.x, n.y, n.z);
  if (positive_finite(nn)) {
    const double sa = vdot(vcross(vsub(C, B), vsub(p, B)), n);
    const double sb = vdot(vcross(vsub(A, C), vsub(p, C)), n);
    const double sc = vdot(vcross(vsub(B, A), vsub(p, A)), n);
    if (sa > 0.0 && sb > 0.0 && sc > 0.0) {
      const double h = __ddiv_rn(vdot(vsub(p, A), n), nn);
      const V3 hn = {mul(h, n.x), mul(h, n.y), mul(h, n.z)};
      const double d2 = dot3(hn.x, hn.y, hn.z);
      if (d2 < best.d2) {
        const double s = add(add(sa, sb), sc);
        const double wa = __ddiv_rn(sa, s), wb = __ddiv_rn(sb, s), wc = __ddiv_rn(sc, s);
        best.d2 = d2;
        best.c = vsub(p, hn);
        best.w[0] = ka == 0 ? wa : (kb == 0 ? wb : wc);
        best.w[1] = ka == 1 ? wa : (kb == 1 ? wb : wc);
        best.w[2] = ka == 2 ? wa : (kb == 2 ? wb : wc);
      }
    }
  }
  if (i0 <= i1) edge_candidate(p, v0, v1, 0, 1, best);
  else edge_candidate(p, v1, v0, 1, 0, best);
  if (i1 <= i2) edge_candidate(p, v1, v2, 1, 2, best);
  else edge_candidate(p, v2, v1, 2, 1, best);
  if (i2 <= i0) edge_candidate(p, v2, v0, 2, 0, best);
  else edge_candidate(p, v0, v2, 0, 2, best);
  return best;
}

// ---- closest point of the mesh ---------------------------------------------------------------------------------------------
// The search keeps (d2, face) only, the smallest pair in that total order, so the result does not depend on the order in
// which cells and faces are met, nor on a face being met in several cells; the winner's point and weights are computed
// once at the end.
__global__ __launch_bounds__(MD_BLOCK) void pc_closest_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  if (t >= a.n_query) return;
  const double* q = a.query + 3 * t;
  const V3 p = {q[0], q[1], q[2]};
  const int64_t out = a.query_idx[t];
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double best_d2 = inf;
  int64_t best_f = -1;
  auto visit = [&](int64_t x, int64_t y, int64_t z) {
    const int64_t row = cell_row(a, pack_key(x, y, z));
    if (row < 0) return;
    const int64_t b = a.cell_start[row], e = b + a.cell_count[row];
    for (int64_t s = b; s < e; ++s) {
      const int64_t f = a.md_cell_face[s];
      if (f == best_f || f < 0 || f >= a.n_faces) continue;   // met again in another cell: the same pair
      const double d2 = face_candidate(a, f, p).d2;
      if (d2 < best_d2 || (d2 == best_d2 && f < best_f)) {
        best_d2 = d2;
        best_f = f;
      }
    }
  };
  ring_walk(a, p.x, p.y, p.z, visit, [&] { return __dsqrt_rn(best_d2); });
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double dist = __dsqrt_rn(best_d2);
  Cand w;
  if (best_f >= 0 && dist <= a.bound) {
    w = face_candidate(a, best_f, p);
  } else {
    dist = inf;
    best_f = -1;
    w.c = {nan, nan, nan};
    w.w[0] = w.w[1] = w.w[2] = nan;
  }
  a.dist[out] = dist;
  a.idx[out] = best_f;
  double* po = a.md_point + 3 * out;
  double* wo = a.md_bary + 3 * out;
  po[0] = w.c.x, po[1] = w.c.y, po[2] = w.c.z;
  wo[0] = w.w[0], wo[1] = w.w[1], wo[2] = w.w[2];
}

// ---- launchers --------------------------------------------------------------------------------------------------------
#define MD_2_31 (1LL << 31)

// what the two binning entry points share; NULL when the descriptor is in order
static const char* tribin_check(const NudfPointCloud& a, bool emit) {
  if (a.n_faces >= MD_2_31 || a.n_verts >= MD_2_31 || a.n_verts < 0) return "n_faces and n_verts must lie in [0, 2^31)";
  if (!(a.cell > 0.0) || !(a.cell < __builtin_inf())) return "cell must be a positive finite number";
  if (!grid_ok(a)) return "grid must lie in [1, 2^21] on every axis";
  if (!origin_ok(a)) return "origin must be finite";
  if (a.cap < 0 || a.cap > MD_MAX_CAP) return "cap must lie in [0, 2^40]";
  if (emit && a.md_n_refs < 0) return "md_n_refs < 0";
  if (!a.verts || !a.faces || !a.md_ref_n) return "NULL verts, faces or md_ref_n";
  if (emit && (!a.md_ref_off || !a.md_ref_key || !a.md_ref_face)) return "NULL md_ref_off, md_ref_key or md_ref_face";
  return nullptr;
}

extern "C" int nudf_pc_tribin_count(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_faces <= 0) return 0;
  if (const char* why = tribin_check(a, false)) return refuse("nudf_pc_tribin_count", why);
  MESH_LAUNCH(pc_tribin_count_kernel, a.n_faces, MD_BLOCK, MD_BLOCK, "nudf_pc_tribin_count");
}

extern "C" int nudf_pc_tribin_emit(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  if (a.n_faces <= 0) return 0;
  if (const char* why = tribin_check(a, true)) return refuse("nudf_pc_tribin_emit", why);
  MESH_LAUNCH(pc_tribin_emit_kernel, a.n_faces, MD_BLOCK, MD_BLOCK, "nudf_pc_tribin_emit");
}

extern "C" int nudf_pc_closest(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_closest";
  if (a.n_query <= 0) return 0;
  if (a.n_query >= MD_2_31 || a.n_faces >= MD_2_31 || a.n_verts >= MD_2_31 || a.n_faces < 0 || a.n_verts < 0)
    return refuse(entry, "n_query, n_faces and n_verts must lie in [0, 2^31)");
  if (!(a.cell > 0.0) || !(a.cell < __builtin_inf())) return refuse(entry, "cell must be a positive finite number");
  if (!grid_ok(a)) return refuse(entry, "grid must lie in [1, 2^21] on every axis");
  if (!origin_ok(a)) return refuse(entry, "origin must be finite");
  if (!(a.bound > 0.0)) return refuse(entry, "bound must be > 0");
  if (a.hash_cap < 2 || (a.hash_cap & (a.hash_cap - 1)) || a.n_cells <= 0 || a.hash_cap < 2 * a.n_cells)
    return refuse(entry, "hash_cap must be a power of two >= 2 n_cells, n_cells > 0");
  if (a.md_n_refs <= 0 || a.n_faces <= 0) return refuse(entry, "no faces or no references to search");
  if (!a.verts || !a.faces || !a.query || !a.query_idx || !a.cell_start || !a.cell_count || !a.hash_key || !a.hash_row ||
      !a.md_cell_face || !a.dist || !a.idx || !a.md_point || !a.md_bary)
    return refuse(entry, "NULL buffer");
  MESH_LAUNCH(pc_closest_kernel, a.n_query, MD_BLOCK, MD_BLOCK, entry);
}
