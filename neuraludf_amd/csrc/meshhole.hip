// Mesh hole closing (include/nudf.h NudfMeshTopo sp_sd_hf_ fields, neuraludf_amd/meshclean.py border_loops /
// close_holes): border loops of any length, defined through the fans of the surface, and their minimum-area
// triangulation (Barequet and Sharir; the area term of Liepa's weight).  What the reference's users leave the GPU for
// after trimesh's fill_holes, which closes loops of 3 and 4 edges only (MeshLab, pymeshfix).
//   link         -- one thread per (border edge, end): the border edge the fan around that end leads to, or -1;
//   rank         -- one thread per directed state: one pointer-doubling round over (jump, smallest id, distance to it);
//   count        -- one thread per loop: perimeter in loop order, the status and the number of triangles;
//   triangulate  -- one wavefront per loop: the dynamic programme over the diagonals in LDS, the refusal of a patch one
//                   of whose diagonals is an edge already, the winding vote and the triangles in pre-order.
// Every thread writes its own item only and sums in list order: no atomics, identical from run to run.  The float64
// expressions follow the numpy restatement (tests/meshhole_ref.py) operation by operation: products and sums go through
// mul / add / sub of f64_exact.h under the pragma; the square roots are the correctly rounded __dsqrt_rn.
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define HF_BLOCK 256
#define HF_WAVE 64
#define HF_MAX NUDF_HOLE_MAX_EDGES
#define HF_FAN_CAP NUDF_HOLE_FAN_CAP

static_assert(HF_MAX == HF_WAVE, "a diagonal's cells and a loop's triangles are spread over one wavefront");

__device__ __forceinline__ bool vertex_ok(const NudfMeshTopo& a, int64_t v) { return v >= 0 && v < a.n_verts; }

// ---- (a) the link of a border edge's end ---------------------------------------------------------------------------------
// the half-edge slots of face t at vertex v other than the one on edge `from`: -1 unless there is exactly one
__device__ __forceinline__ int64_t other_edge_at(const NudfMeshTopo& a, int64_t f, const int64_t* t, int64_t v, int64_t from) {
  int64_t found = -1;
  int n = 0;
  for (int k = 0; k < 3; ++k) {
    if (t[k] != v && t[(k + 1) % 3] != v) continue;
    const int64_t e = a.he_edge[3 * f + k];
    if (e == from) continue;
    found = e;
    ++n;
  }
  return n == 1 ? found : -1;
}

__global__ __launch_bounds__(HF_BLOCK) void hf_link_kernel(NudfMeshTopo a) {
  const int64_t s = (int64_t)blockIdx.x * HF_BLOCK + threadIdx.x;
  if (s >= 2 * a.sp_sd_hf_n_border) return;
  int64_t out = -1;
  const int64_t e0 = a.sp_sd_hf_bedge[s >> 1];
  if (e0 >= 0 && e0 < a.n_edges && a.edges[5 * e0 + 2] == 1) {
    const int64_t v = a.edges[5 * e0 + (s & 1)];
    const int64_t f0 = a.edges[5 * e0 + 3];
    int64_t f = f0, e = e0;
    for (int step = 0; step < HF_FAN_CAP; ++step) {
      if (f < 0 || f >= a.n_faces) break;
      const int64_t* t = a.faces + 3 * f;
      if (t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) break;                  // a face with a repeated vertex blocks
      const int64_t ne = other_edge_at(a, f, t, v, e);
      if (ne < 0 || ne >= a.n_edges) break;
      const int64_t* row = a.edges + 5 * ne;
      if (row[2] == 1) {                                                          // the linked border edge
        const int64_t b = a.sp_sd_hf_brank[ne];
        if (b >= 0 && b < a.sp_sd_hf_n_border && ne != e0 && row[0] != row[1]) out = 2 * b + (row[1] == v ? 1 : 0);
        break;
      }
      if (row[2] != 2) break;                                                     // three faces or more: blocked
      const int64_t nf = row[3] == f ? row[4] : (row[4] == f ? row[3] : -1);
      if (nf == f0 || nf == f) break;
      f = nf;
      e = ne;
    }
  }
  a.sp_sd_hf_link[s] = out;
}

// ---- (b) one pointer-doubling round --------------------------------------------------------------------------------------
__global__ __launch_bounds__(HF_BLOCK) void hf_rank_kernel(NudfMeshTopo a) {
  const int64_t s = (int64_t)blockIdx.x * HF_BLOCK + threadIdx.x;
  const int64_t n = 2 * a.sp_sd_hf_n_border;
  if (s >= n) return;
  const int64_t* in = a.sp_sd_hf_rank_in + 3 * s;
  int64_t* o = a.sp_sd_hf_rank_out + 3 * s;
  const int64_t j = in[0];
  o[0] = j;
  o[1] = in[1];
  o[2] = in[2];
  if (j < 0 || j >= n) return;
  const int64_t* nx = a.sp_sd_hf_rank_in + 3 * j;
  o[0] = nx[0];
  if (nx[1] < in[1]) {                                          // strictly smaller: the first occurrence keeps the place
    o[1] = nx[1];
    o[2] = ((int64_t)1 << a.sp_sd_hf_round) + nx[2];
  }
}

// ---- (c) perimeter, status and triangle count of a loop -----------------------------------------------------------------
// the loop's CSR range [b, b + n) when it lies inside the tables, else n = -1
__device__ __forceinline__ int64_t loop_range(const NudfMeshTopo& a, int64_t l, int64_t* b) {
  *b = a.sp_sd_hf_loop_off[l];
  const int64_t e = a.sp_sd_hf_loop_off[l + 1];
  return *b >= 0 && e >= *b && e <= a.sp_sd_hf_n_items ? e - *b : -1;
}

__device__ __forceinline__ bool finite3(const double* p) { return is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]); }

__global__ __launch_bounds__(HF_BLOCK) void hf_count_kernel(NudfMeshTopo a) {
  const int64_t l = (int64_t)blockIdx.x * HF_BLOCK + threadIdx.x;
  if (l >= a.sp_sd_hf_n_loops) return;
  int64_t b;
  const int64_t n = loop_range(a, l, &b);
  double per = 0.0;
  bool tables = n >= 0, finite = true;
  for (int64_t i = 0; tables && i < n; ++i) {                   // every loop, whatever its length: in loop order
    const int64_t e = a.sp_sd_hf_loop_edge[b + i], w = a.sp_sd_hf_loop_vertex[b + i];
    if (e < 0 || e >= a.n_edges || !vertex_ok(a, w)) { tables = false; break; }
    const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1];
    if (!vertex_ok(a, u) || !vertex_ok(a, v)) { tables = false; break; }
    const double *p = a.pos + 3 * u, *q = a.pos + 3 * v;
    finite = finite && finite3(a.pos + 3 * w) && finite3(p) && finite3(q);
    const double len = __dsqrt_rn(dot3(sub(p[0], q[0]), sub(p[1], q[1]), sub(p[2], q[2])));
    per = i == 0 ? len : add(per, len);
  }
  int status = NUDF_HOLE_FILLED;
  if (!tables) {
    status = NUDF_HOLE_NONFINITE;
    per = NAN;
  } else if (!a.sp_sd_hf_closed[l]) {
    status = NUDF_HOLE_OPEN_CHAIN;
  } else if (n < 3 || n > a.max_loop) {
    status = NUDF_HOLE_TOO_MANY_EDGES;
  } else {
    bool twice = false;
    for (int64_t i = 1; i < n; ++i)
      for (int64_t j = 0; j < i; ++j) twice = twice || a.sp_sd_hf_loop_vertex[b + i] == a.sp_sd_hf_loop_vertex[b + j];
    if (twice) status = NUDF_HOLE_REPEATED_VERTEX;
    else if (!finite || !is_finite(per)) status = NUDF_HOLE_NONFINITE;
    else if (per > a.sp_sd_hf_max_perimeter) status = NUDF_HOLE_PERIMETER;
  }
  a.sp_sd_hf_perimeter[l] = per;
  a.sp_sd_hf_status[l] = (int8_t)status;
  a.new_count[l] = status == NUDF_HOLE_FILLED ? n - 2 : 0;
}

// ---- (d) the minimum-area triangulation ----------------------------------------------------------------------------------
// mul(0.5, sqrt(dot3(cross(q - p, r - p))))
__device__ __forceinline__ double tri_area(const V3& p, const V3& q, const V3& r) {
  const V3 c = vcross(vsub(q, p), vsub(r, p));
  return mul(0.5, __dsqrt_rn(dot3(c.x, c.y, c.z)));
}

// position of `key` in the ascending edge_key, or -1
__device__ __forceinline__ int64_t find_edge(const NudfMeshTopo& a, int64_t key) {
  int64_t lo = 0, hi = a.n_edges;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a.edge_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.n_edges && a.edge_key[lo] == key ? lo : -1;
}

__global__ __launch_bounds__(HF_WAVE) void hf_triangulate_kernel(NudfMeshTopo a) {
  __shared__ double W[HF_MAX * HF_MAX];                 // 32 KB
  __shared__ uint8_t split[HF_MAX * HF_MAX];            //  4 KB
  __shared__ double P[HF_MAX * 3];
  __shared__ int64_t vid[HF_MAX];
  __shared__ uint8_t tri[HF_MAX][3];                    // the triangles (i, k, j) in pre-order
  __shared__ uint8_t stack[HF_MAX][2];
  __shared__ uint8_t along[HF_MAX];
  __shared__ int verdict[3];                            // ok, refuse, flip

  const int64_t l = blockIdx.x;
  const int lane = threadIdx.x;
  if (a.sp_sd_hf_status[l] != NUDF_HOLE_FILLED) return;               // the whole block leaves: no barrier is skipped
  int64_t b;
  const int64_t n64 = loop_range(a, l, &b);
  const int64_t out = a.new_off[l];
  if (n64 < 3 || n64 > HF_MAX || n64 > a.max_loop || out < 0 || out + n64 - 2 > a.n_new) return;
  const int n = (int)n64;

  // stage the loop; an index outside the tables refuses it
  if (lane == 0) verdict[0] = 1, verdict[1] = 0, verdict[2] = 0;
  __syncthreads();
  int same = 0;
  if (lane < n) {
    const int64_t v = a.sp_sd_hf_loop_vertex[b + lane], e = a.sp_sd_hf_loop_edge[b + lane];
    bool ok = vertex_ok(a, v) && e >= 0 && e < a.n_edges;
    if (ok) {
      vid[lane] = v;
      for (int c = 0; c < 3; ++c) P[3 * lane + c] = a.pos[3 * v + c];
      // does the face on this border edge run along it in loop direction?
      const int64_t f = a.edges[5 * e + 3];
      ok = f >= 0 && f < a.n_faces;
      if (ok)
        for (int k = 0; k < 3; ++k)
          if (a.he_edge[3 * f + k] == e) same = a.faces[3 * f + k] == v;
    }
    if (!ok) verdict[0] = 0;
    along[lane] = (uint8_t)same;
    W[lane * HF_MAX + (lane + 1) % HF_MAX] = 0.0;
  }
  __syncthreads();
  if (!verdict[0]) return;

  // the diagonals in order, the cells of one across the lanes
  for (int d = 2; d < n; ++d) {
    const int i = lane, j = lane + d;
    if (j < n) {
      const V3 pi = vload(P + 3 * i), pj = vload(P + 3 * j);
      double best = 0.0;
      int arg = i + 1;
      for (int k = i + 1; k < j; ++k) {
        const double w = add(add(W[i * HF_MAX + k], W[k * HF_MAX + j]), tri_area(pi, vload(P + 3 * k), pj));
        if (k == i + 1 || w < best) best = w, arg = k;
      }
      W[i * HF_MAX + j] = best;
      split[i * HF_MAX + j] = (uint8_t)arg;
    }
    __syncthreads();
  }

  // one lane: the pre-order descent from (0, n - 1) and the vote
  if (lane == 0) {
    int top = 0, m = 0, votes = 0;
    stack[top][0] = 0, stack[top][1] = (uint8_t)(n - 1), ++top;
    while (top > 0 && m < n - 2) {
      --top;
      const int i = stack[top][0], j = stack[top][1];
      if (j - i < 2) continue;
      const int k = split[i * HF_MAX + j];
      tri[m][0] = (uint8_t)i, tri[m][1] = (uint8_t)k, tri[m][2] = (uint8_t)j, ++m;
      if (top + 2 > HF_MAX) break;
      stack[top][0] = (uint8_t)k, stack[top][1] = (uint8_t)j, ++top;
      stack[top][0] = (uint8_t)i, stack[top][1] = (uint8_t)k, ++top;
    }
    for (int i = 0; i < n; ++i) votes += along[i];
    verdict[0] = m == n - 2;
    verdict[2] = 2 * votes > n;                                   // the patch runs against the majority of its neighbours
  }
  __syncthreads();
  if (!verdict[0]) return;

  // refusal: triangle t spans the chord (i, j), a diagonal unless it is the root's
  bool mine = false;
  int ti = 0, tk = 0, tj = 0;
  if (lane < n - 2) {
    ti = tri[lane][0], tk = tri[lane][1], tj = tri[lane][2];
    mine = true;
    if (!(ti == 0 && tj == n - 1)) {
      const int64_t u = vid[ti], v = vid[tj];
      if (find_edge(a, (u < v ? u : v) * a.n_verts + (u < v ? v : u)) >= 0) verdict[1] = 1;
    } else if (n == 3) {                                          // the triangle is a face already: an island of one face
      const int64_t f0 = a.edges[5 * a.sp_sd_hf_loop_edge[b] + 3], f1 = a.edges[5 * a.sp_sd_hf_loop_edge[b + 1] + 3],
                    f2 = a.edges[5 * a.sp_sd_hf_loop_edge[b + 2] + 3];
      if (f0 == f1 && f1 == f2) verdict[1] = 1;
    }
  }
  __syncthreads();
  const bool refused = verdict[1] != 0;
  if (refused && lane == 0) a.sp_sd_hf_status[l] = NUDF_HOLE_DUPLICATE;
  if (!mine) return;
  int64_t* o = a.new_faces + 3 * (out + lane);
  const bool flip = verdict[2] != 0;
  o[0] = refused ? -1 : vid[ti];
  o[1] = refused ? -1 : vid[flip ? tj : tk];
  o[2] = refused ? -1 : vid[flip ? tk : tj];
}

// ---- launchers --------------------------------------------------------------------------------------------------------
// the counts every entry point is handed; NULL when they are in order, else what is wrong
static const char* bad_sizes(const NudfMeshTopo& a) {
  const int64_t lim = 1LL << 31;
  if (a.n_faces < 0 || a.n_faces >= lim) return "n_faces must be in [0, 2^31)";
  if (a.n_verts < 0 || a.n_verts >= lim) return "n_verts must be in [0, 2^31)";
  if (a.n_edges < 0 || a.n_edges > 3 * a.n_faces) return "n_edges must be in [0, 3 n_faces]";
  if (a.sp_sd_hf_n_border < 0 || a.sp_sd_hf_n_border > a.n_edges) return "sp_sd_hf_n_border must be in [0, n_edges]";
  if (a.sp_sd_hf_n_loops < 0 || a.sp_sd_hf_n_loops > a.sp_sd_hf_n_border) return "sp_sd_hf_n_loops must be in [0, sp_sd_hf_n_border]";
  if (a.sp_sd_hf_n_items < 0 || a.sp_sd_hf_n_items > a.sp_sd_hf_n_border) return "sp_sd_hf_n_items must be in [0, sp_sd_hf_n_border]";
  if (a.n_new < 0 || a.n_new > a.sp_sd_hf_n_border) return "n_new must be in [0, sp_sd_hf_n_border]";
  return nullptr;
}

static const char* bad_max_edges(const NudfMeshTopo& a) {
  return a.max_loop >= 3 && a.max_loop <= HF_MAX ? nullptr : "max_loop (the longest loop to close) must be in [3, 64]";
}

extern "C" int nudf_meshhole_link(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshhole_link";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.sp_sd_hf_n_border <= 0) return 0;
  if (!a.faces || !a.edges || !a.he_edge || !a.sp_sd_hf_bedge || !a.sp_sd_hf_brank || !a.sp_sd_hf_link)
    return refuse(entry, "NULL faces, edges, he_edge, sp_sd_hf_bedge, sp_sd_hf_brank or sp_sd_hf_link");
  MESH_LAUNCH(hf_link_kernel, 2 * a.sp_sd_hf_n_border, HF_BLOCK, HF_BLOCK, entry);
}

extern "C" int nudf_meshhole_rank(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshhole_rank";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.sp_sd_hf_round < 0 || a.sp_sd_hf_round > 40) return refuse(entry, "sp_sd_hf_round must be in [0, 40]");
  if (a.sp_sd_hf_n_border <= 0) return 0;
  if (!a.sp_sd_hf_rank_in || !a.sp_sd_hf_rank_out) return refuse(entry, "NULL sp_sd_hf_rank_in or sp_sd_hf_rank_out");
  if (a.sp_sd_hf_rank_in == a.sp_sd_hf_rank_out) return refuse(entry, "sp_sd_hf_rank_in and sp_sd_hf_rank_out must differ");
  MESH_LAUNCH(hf_rank_kernel, 2 * a.sp_sd_hf_n_border, HF_BLOCK, HF_BLOCK, entry);
}

extern "C" int nudf_meshhole_count(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshhole_count";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.sp_sd_hf_n_loops <= 0) return 0;
  if (const char* why = bad_max_edges(a)) return refuse(entry, why);
  if (!(a.sp_sd_hf_max_perimeter > 0.0)) return refuse(entry, "sp_sd_hf_max_perimeter must be positive (+inf: no bound)");
  if (!a.edges || !a.pos || !a.sp_sd_hf_loop_off || !a.sp_sd_hf_loop_vertex || !a.sp_sd_hf_loop_edge || !a.sp_sd_hf_closed ||
      !a.sp_sd_hf_perimeter || !a.sp_sd_hf_status || !a.new_count)
    return refuse(entry, "NULL edges, pos, sp_sd_hf_loop_off, sp_sd_hf_loop_vertex, sp_sd_hf_loop_edge, sp_sd_hf_closed, "
                         "sp_sd_hf_perimeter, sp_sd_hf_status or new_count");
  MESH_LAUNCH(hf_count_kernel, a.sp_sd_hf_n_loops, HF_BLOCK, HF_BLOCK, entry);
}

extern "C" int nudf_meshhole_triangulate(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshhole_triangulate";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.sp_sd_hf_n_loops <= 0 || a.n_new <= 0) return 0;
  if (const char* why = bad_max_edges(a)) return refuse(entry, why);
  if (!a.faces || !a.edges || !a.he_edge || !a.edge_key || !a.pos || !a.sp_sd_hf_loop_off || !a.sp_sd_hf_loop_vertex ||
      !a.sp_sd_hf_loop_edge || !a.sp_sd_hf_status || !a.new_off || !a.new_faces)
    return refuse(entry, "NULL faces, edges, he_edge, edge_key, pos, sp_sd_hf_loop_off, sp_sd_hf_loop_vertex, "
                         "sp_sd_hf_loop_edge, sp_sd_hf_status, new_off or new_faces");
  MESH_LAUNCH(hf_triangulate_kernel, a.sp_sd_hf_n_loops, HF_WAVE, 1, entry);
}
