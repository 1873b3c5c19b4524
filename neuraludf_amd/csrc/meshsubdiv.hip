// Mesh subdivision (include/nudf.h NudfMeshTopo sp_sd_ fields, neuraludf_amd/meshclean.py subdivide_mesh /
// subdivide_to_edge): what the reference's users leave the GPU for to make a mesh finer (trimesh.remesh.subdivide,
// subdivide_loop, subdivide_to_size; open3d's subdivide_midpoint / subdivide_loop).
//   mark   -- one thread per unique edge: split it when it is longer than the bound, or always;
//   odd    -- one thread per marked edge: the new vertex, the midpoint or Loop's 3/8 3/8 1/8 1/8 stencil;
//   even   -- one thread per old vertex: a copy, or Loop's vertex rule with Warren's weights (border: 3/4 1/8 1/8);
//   count  -- one thread per face: 1 + its marked half-edges;
//   emit   -- one thread per face: the children of the 0 / 1 / 2 / 3-marked template, in the parent's winding.
// Every thread writes its own item only and sums in list order: no atomics, identical from run to run.  The float64
// expressions follow the numpy restatement (tests/meshsubdiv_ref.py) operation by operation: products and sums go through
// mul / add / sub of f64_exact.h under the pragma; the one division is Warren's 3 / (8 n).
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define SD_BLOCK 256

__device__ __forceinline__ bool vertex_ok(const NudfMeshTopo& a, int64_t v) { return v >= 0 && v < a.n_verts; }

__device__ __forceinline__ bool in_range(const NudfMeshTopo& a, const int64_t* t) {
  return vertex_ok(a, t[0]) && vertex_ok(a, t[1]) && vertex_ok(a, t[2]);
}

// (dx dx + dy dy) + dz dz of two rows of three
__device__ __forceinline__ double dist2(const double* p, const double* q) {
  const double dx = sub(p[0], q[0]), dy = sub(p[1], q[1]), dz = sub(p[2], q[2]);
  return add(add(mul(dx, dx), mul(dy, dy)), mul(dz, dz));
}

// ---- (a) which edges are split -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_BLOCK) void sd_mark_kernel(NudfMeshTopo a) {
  const int64_t e = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
  if (e >= a.n_edges) return;
  const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1];
  uint8_t m = 0;
  if (u != v && vertex_ok(a, u) && vertex_ok(a, v))
    m = a.sp_sd_mark_all ? 1 : dist2(a.pos + 3 * u, a.pos + 3 * v) > mul(a.sp_sd_max_edge, a.sp_sd_max_edge);
  a.sp_sd_mark[e] = m;
}

// ---- (b) the new vertices ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double midpoint(double pu, double pv) { return mul(add(pu, pv), 0.5); }
__device__ __forceinline__ double loop_odd(double pu, double pv, double pa, double pb) {
  return add(mul(add(pu, pv), 0.375), mul(add(pa, pb), 0.125));
}

// the vertex opposite half-edge h in its face, or -1
__device__ __forceinline__ int64_t opposite(const NudfMeshTopo& a, int64_t h) {
  if (h < 0 || h >= 3 * a.n_faces) return -1;
  const int64_t w = a.faces[h / 3 * 3 + (h % 3 + 2) % 3];
  return vertex_ok(a, w) ? w : -1;
}

__global__ __launch_bounds__(SD_BLOCK) void sd_odd_kernel(NudfMeshTopo a) {
  const int64_t j = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
  if (j >= a.sp_sd_n_marked) return;
  const int64_t row = a.n_verts + j;
  const int W = a.sp_attr_width;
  double* o = a.sp_sd_pos_out + 3 * row;
  double* oa = W > 0 ? a.sp_sd_attr_out + (int64_t)W * row : nullptr;
  o[0] = o[1] = o[2] = 0.0;
  for (int c = 0; c < W; ++c) oa[c] = 0.0;
  const int64_t e = a.sp_sd_marked[j];
  if (e < 0 || e >= a.n_edges) return;
  const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1];
  if (!vertex_ok(a, u) || !vertex_ok(a, v)) return;
  int64_t wa = -1, wb = -1;
  if (a.sp_sd_scheme == 1 && a.edges[5 * e + 2] == 2) {
    const int64_t s = a.edge_start[e];
    if (s >= 0 && s + 1 < 3 * a.n_faces) {
      wa = opposite(a, a.he_id[s]);
      wb = opposite(a, a.he_id[s + 1]);
    }
  }
  const bool smooth = wa >= 0 && wb >= 0;
  const double *pu = a.pos + 3 * u, *pv = a.pos + 3 * v;
  const double *pa = smooth ? a.pos + 3 * wa : pu, *pb = smooth ? a.pos + 3 * wb : pv;
  for (int c = 0; c < 3; ++c) o[c] = smooth ? loop_odd(pu[c], pv[c], pa[c], pb[c]) : midpoint(pu[c], pv[c]);
  if (W > 0) {
    const double *qu = a.sp_attr + (int64_t)W * u, *qv = a.sp_attr + (int64_t)W * v;
    const double *qa = smooth ? a.sp_attr + (int64_t)W * wa : qu, *qb = smooth ? a.sp_attr + (int64_t)W * wb : qv;
    for (int c = 0; c < W; ++c) oa[c] = smooth ? loop_odd(qu[c], qv[c], qa[c], qb[c]) : midpoint(qu[c], qv[c]);
  }
}

// ---- (c) the old vertices ------------------------------------------------------------------------------------------------
// one column of Loop's vertex rule: p w + s beta, s over the ring [b, e) in list order from its first entry
__device__ __forceinline__ double ring_rule(const int64_t* ring, int64_t b, int64_t e, const double* src, int64_t stride, int c,
                                            double p, double w, double beta) {
  double s = src[stride * ring[b] + c];
  for (int64_t j = b + 1; j < e; ++j) s = add(s, src[stride * ring[j] + c]);
  return add(mul(p, w), mul(s, beta));
}

__device__ __forceinline__ double border_rule(double p, double q0, double q1) { return add(mul(p, 0.75), mul(add(q0, q1), 0.125)); }

__global__ __launch_bounds__(SD_BLOCK) void sd_even_kernel(NudfMeshTopo a) {
  const int64_t v = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  const int W = a.sp_attr_width;
  const double* p = a.pos + 3 * v;
  double* o = a.sp_sd_pos_out + 3 * v;
  const double* q = W > 0 ? a.sp_attr + (int64_t)W * v : nullptr;
  double* oa = W > 0 ? a.sp_sd_attr_out + (int64_t)W * v : nullptr;
  for (int c = 0; c < 3; ++c) o[c] = p[c];
  for (int c = 0; c < W; ++c) oa[c] = q[c];
  if (a.sp_sd_scheme != 1) return;
  const int cls = a.sp_sd_vclass[v];
  if (cls == 1) {
    const int64_t b = a.nbr_off[v], e = a.nbr_off[v + 1];
    if (b < 0 || e > a.sp_sd_n_border || e - b != 2) return;
    const int64_t b0 = a.nbr[b], b1 = a.nbr[b + 1];
    if (!vertex_ok(a, b0) || !vertex_ok(a, b1)) return;
    for (int c = 0; c < 3; ++c) o[c] = border_rule(p[c], a.pos[3 * b0 + c], a.pos[3 * b1 + c]);
    for (int c = 0; c < W; ++c) oa[c] = border_rule(q[c], a.sp_attr[(int64_t)W * b0 + c], a.sp_attr[(int64_t)W * b1 + c]);
  } else if (cls == 0) {
    const int64_t b = a.sp_sd_ring_off[v], e = a.sp_sd_ring_off[v + 1];
    if (b < 0 || e > a.sp_sd_n_ring || e <= b) return;
    for (int64_t j = b; j < e; ++j)
      if (!vertex_ok(a, a.sp_sd_ring[j])) return;
    const int64_t n = e - b;
    const double nd = (double)n;
    const double beta = n == 3 ? 0.1875 : __ddiv_rn(3.0, mul(8.0, nd));
    const double w = sub(1.0, mul(nd, beta));
    for (int c = 0; c < 3; ++c) o[c] = ring_rule(a.sp_sd_ring, b, e, a.pos, 3, c, p[c], w, beta);
    for (int c = 0; c < W; ++c) oa[c] = ring_rule(a.sp_sd_ring, b, e, a.sp_attr, W, c, q[c], w, beta);
  }
}

// ---- (d) the faces -------------------------------------------------------------------------------------------------------
// m[k] = the new vertex of half-edge 3 f + k or -1 -> the number of marked half-edges; a face out of range has none
__device__ __forceinline__ int face_marks(const NudfMeshTopo& a, int64_t f, int64_t* m) {
  m[0] = m[1] = m[2] = -1;
  if (!in_range(a, a.faces + 3 * f)) return 0;
  int n = 0;
  for (int k = 0; k < 3; ++k) {
    const int64_t e = a.he_edge[3 * f + k];
    if (e < 0 || e >= a.n_edges) continue;
    const int64_t w = a.sp_sd_edge_vertex[e];
    if (w < a.n_verts || w >= a.n_verts + a.sp_sd_n_marked) continue;
    m[k] = w;
    ++n;
  }
  return n;
}

__global__ __launch_bounds__(SD_BLOCK) void sd_count_kernel(NudfMeshTopo a) {
  const int64_t f = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  int64_t m[3];
  a.sp_sd_fcount[f] = 1 + face_marks(a, f, m);
}

__device__ __forceinline__ void put(const NudfMeshTopo& a, int64_t i, int64_t f, int64_t x, int64_t y, int64_t z) {
  int64_t* o = a.sp_sd_faces_out + 3 * i;
  o[0] = x;
  o[1] = y;
  o[2] = z;
  a.sp_sd_parent[i] = f;
}

__global__ __launch_bounds__(SD_BLOCK) void sd_emit_kernel(NudfMeshTopo a) {
  const int64_t f = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  int64_t m[3];
  const int n = face_marks(a, f, m);
  const int64_t i = a.sp_sd_foff[f];
  if (i < 0 || i + n + 1 > a.sp_sd_n_out) return;
  const int64_t* t = a.faces + 3 * f;
  if (n == 0) {
    put(a, i, f, t[0], t[1], t[2]);
  } else if (n == 1) {
    const int k = m[0] >= 0 ? 0 : (m[1] >= 0 ? 1 : 2);
    const int64_t va = t[k], vb = t[(k + 1) % 3], vc = t[(k + 2) % 3];
    put(a, i, f, va, m[k], vc);
    put(a, i + 1, f, m[k], vb, vc);
  } else if (n == 2) {
    const int k = m[0] < 0 ? 0 : (m[1] < 0 ? 1 : 2);
    const int64_t va = t[k], vb = t[(k + 1) % 3], vc = t[(k + 2) % 3], m1 = m[(k + 1) % 3], m2 = m[(k + 2) % 3];
    put(a, i, f, m1, vc, m2);
    const double da = dist2(a.sp_sd_pos_out + 3 * va, a.sp_sd_pos_out + 3 * m1);
    const double db = dist2(a.sp_sd_pos_out + 3 * vb, a.sp_sd_pos_out + 3 * m2);
    const bool along_a = da < db || (!(da > db) && va < vb);
    if (along_a) {
      put(a, i + 1, f, va, vb, m1);
      put(a, i + 2, f, va, m1, m2);
    } else {
      put(a, i + 1, f, va, vb, m2);
      put(a, i + 2, f, vb, m1, m2);
    }
  } else {
    put(a, i, f, t[0], m[0], m[2]);
    put(a, i + 1, f, m[0], t[1], m[1]);
    put(a, i + 2, f, m[2], m[1], t[2]);
    put(a, i + 3, f, m[0], m[1], m[2]);
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------------
// the counts every entry point is handed; NULL when they are in order, else what is wrong
static const char* bad_sizes(const NudfMeshTopo& a) {
  const int64_t lim = 1LL << 31;
  if (a.n_faces < 0 || a.n_faces >= lim) return "n_faces must be in [0, 2^31)";
  if (a.n_verts < 0 || a.n_verts >= lim) return "n_verts must be in [0, 2^31)";
  if (a.n_edges < 0 || a.n_edges > 3 * a.n_faces) return "n_edges must be in [0, 3 n_faces]";
  if (a.sp_sd_n_marked < 0 || a.sp_sd_n_marked > a.n_edges) return "sp_sd_n_marked must be in [0, n_edges]";
  if (a.n_verts + a.sp_sd_n_marked >= lim) return "n_verts + sp_sd_n_marked must stay below 2^31";
  if (a.sp_sd_n_out < 0 || a.sp_sd_n_out > 4 * a.n_faces) return "sp_sd_n_out must be in [0, 4 n_faces]";
  if (a.sp_sd_n_ring < 0) return "sp_sd_n_ring must be >= 0";
  if (a.sp_sd_n_border < 0) return "sp_sd_n_border must be >= 0";
  if (a.sp_attr_width < 0) return "sp_attr_width must be >= 0";
  return nullptr;
}

static const char* bad_scheme(const NudfMeshTopo& a) {
  return a.sp_sd_scheme == 0 || a.sp_sd_scheme == 1 ? nullptr : "sp_sd_scheme must be 0 (midpoint) or 1 (loop)";
}

extern "C" int nudf_meshsubdiv_mark(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsubdiv_mark";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_edges <= 0) return 0;
  if (!a.sp_sd_mark_all && !(a.sp_sd_max_edge > 0.0 && a.sp_sd_max_edge < HUGE_VAL))
    return refuse(entry, "sp_sd_max_edge must be positive and finite unless sp_sd_mark_all is set");
  if (!a.edges || !a.sp_sd_mark || (!a.sp_sd_mark_all && !a.pos)) return refuse(entry, "NULL edges, sp_sd_mark or pos");
  MESH_LAUNCH(sd_mark_kernel, a.n_edges, SD_BLOCK, SD_BLOCK, entry);
}

extern "C" int nudf_meshsubdiv_odd(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsubdiv_odd";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.sp_sd_n_marked <= 0) return 0;
  if (const char* why = bad_scheme(a)) return refuse(entry, why);
  if (!a.sp_sd_marked || !a.edges || !a.pos || !a.sp_sd_pos_out) return refuse(entry, "NULL sp_sd_marked, edges, pos or sp_sd_pos_out");
  if (a.sp_attr_width > 0 && (!a.sp_attr || !a.sp_sd_attr_out)) return refuse(entry, "NULL sp_attr or sp_sd_attr_out");
  if (a.sp_sd_scheme == 1 && (!a.faces || !a.he_id || !a.edge_start)) return refuse(entry, "NULL faces, he_id or edge_start");
  MESH_LAUNCH(sd_odd_kernel, a.sp_sd_n_marked, SD_BLOCK, SD_BLOCK, entry);
}

extern "C" int nudf_meshsubdiv_even(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsubdiv_even";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_verts <= 0) return 0;
  if (const char* why = bad_scheme(a)) return refuse(entry, why);
  if (!a.pos || !a.sp_sd_pos_out) return refuse(entry, "NULL pos or sp_sd_pos_out");
  if (a.sp_attr_width > 0 && (!a.sp_attr || !a.sp_sd_attr_out)) return refuse(entry, "NULL sp_attr or sp_sd_attr_out");
  if (a.sp_sd_scheme == 1 && (!a.sp_sd_vclass || !a.sp_sd_ring_off || !a.nbr_off || (a.sp_sd_n_ring > 0 && !a.sp_sd_ring) ||
                              (a.sp_sd_n_border > 0 && !a.nbr)))
    return refuse(entry, "NULL sp_sd_vclass, sp_sd_ring_off, sp_sd_ring, nbr_off or nbr");
  MESH_LAUNCH(sd_even_kernel, a.n_verts, SD_BLOCK, SD_BLOCK, entry);
}

extern "C" int nudf_meshsubdiv_count(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsubdiv_count";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_faces <= 0) return 0;
  if (!a.faces || !a.he_edge || !a.sp_sd_edge_vertex || !a.sp_sd_fcount)
    return refuse(entry, "NULL faces, he_edge, sp_sd_edge_vertex or sp_sd_fcount");
  MESH_LAUNCH(sd_count_kernel, a.n_faces, SD_BLOCK, SD_BLOCK, entry);
}

extern "C" int nudf_meshsubdiv_emit(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsubdiv_emit";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_faces <= 0) return 0;
  if (!a.faces || !a.he_edge || !a.sp_sd_edge_vertex || !a.sp_sd_foff || !a.sp_sd_faces_out || !a.sp_sd_parent || !a.sp_sd_pos_out)
    return refuse(entry, "NULL faces, he_edge, sp_sd_edge_vertex, sp_sd_foff, sp_sd_faces_out, sp_sd_parent or sp_sd_pos_out");
  MESH_LAUNCH(sd_emit_kernel, a.n_faces, SD_BLOCK, SD_BLOCK, entry);
}
