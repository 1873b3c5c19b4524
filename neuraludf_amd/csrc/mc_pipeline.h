// The marching-cubes pipeline of the four meshers (meshudf.hip, meshudf_sparse.hip, isosurface.hip): grid numbering, brick
// lookup, the seven kernels and their host wrappers, written once and parameterised on the argument struct of
// include/nudf.h (passed to the kernels by value) and on a rule, the only thing that differs between the meshers.
//   dense   classify  -- one thread per cell, consecutive threads along k (the contiguous grid axis): case index, triangle
//                        count, and a 1 stored at every sign-change edge of a cell that emits triangles;
//           emit      -- one thread per cell with triangles: its faces at the caller's exclusive scan of the counts,
//                        vertex indices from the caller's inclusive scan of the edge flags;
//           vertices  -- one thread per flagged edge;
//   sparse  classify  -- one workgroup per brick, the brick's (B+1)^3 values staged in LDS (each is a corner of up to 8
//                        cells): case index and triangle count per brick cell;
//           edges     -- one thread per cell with triangles (the caller's ascending list of global cell indices): the
//                        global id of each of its sign-change edges, INT64_MAX for the other edges; the caller sorts and
//                        uniques them;
//           emit      -- as dense; the vertex of an edge = the position of its id in the sorted unique edge array;
//           vertices  -- one thread per unique edge: the end values come from a selected brick that holds both ends, found
//                        through block_slot (every copy of a shared node holds the same bits).
// A rule is built from the argument struct and gives cell_case(8 corner values, corner -> storage index, nt) and
// weight(lower end value, upper end value); the field (U or F) comes from the struct's mc_field overload, declared by the
// translation unit.  No atomics: every output position is a function of the inputs alone, so a mesh is identical from run
// to run and the sparse meshers reproduce the dense ones bit for bit.  Dense cell indices fit 32 bits ((N-1)^3 < 2^30 for
// N <= 1024); grid point, edge and sparse cell ids are 64-bit (3 N^3 = 2^37.6 at N = 4096); block ids fit 32 bits.
#pragma once
#include <climits>
#include "nudf_common.h"
#include "../../include/nudf.h"
#include "mc_tables.inc"
#include "isosurface_cell.h"

#define MC_BLOCK 256
#define MC_MIN_N 3
#define MC_DENSE_MAX_N 1024
#define MC_SPARSE_MAX_N 4096

// ---- rules -------------------------------------------------------------------------------------------------------------

// MeshUDF: pseudo-signs from the gradients of active cells (meshudf_cell.h); G is stored like the field, and the storage
// indices cell_case is given count from `origin` (a brick's first node in the sparse kernels)
struct McUdfRule {
  const float* G;
  float mean_thr, max_thr;
  template <class A>
  __device__ explicit McUdfRule(const A& a, int64_t origin = 0) : G(a.G + 3 * origin), mean_thr(a.mean_thr), max_thr(a.max_thr) {}
  template <class Index>
  __device__ uint32_t cell_case(const float (&u)[8], Index index, uint32_t& nt) const {
    return meshudf_cell_case(u, mean_thr, max_thr, [&](int c) { return G + 3 * index(c); }, nt);
  }
  __device__ float weight(float ua, float ub) const { return meshudf_vertex_weight(ua, ub); }
};

// level set: corner c is `-` iff F_c < level (isosurface_cell.h)
struct McLevelRule {
  float level;
  template <class A>
  __device__ explicit McLevelRule(const A& a, int64_t = 0) : level(a.level) {}
  template <class Index>
  __device__ uint32_t cell_case(const float (&f)[8], Index, uint32_t& nt) const { return iso_cell_case(f, level, nt); }
  __device__ float weight(float fa, float fb) const { return iso_vertex_weight(fa, fb, level); }
};

// ---- grid numbering ----------------------------------------------------------------------------------------------------

// offset of corner c of a cell from its lowest corner in an array of n nodes per axis (corner bits: 4 = x, 2 = y, 1 = z;
// neuraludf_amd/mc_tables.py)
template <class I>
__device__ __forceinline__ I mc_corner_offset(int c, I n) {
  return ((c >> 2) & 1) * n * n + ((c >> 1) & 1) * n + (c & 1);
}

// lowest grid point of compact cell index `cell` of the dense grid
__device__ __forceinline__ int64_t mc_cell_base(uint32_t cell, uint32_t M, int64_t N) {
  const uint32_t k = cell % M, r = cell / M;
  const uint32_t j = r % M, i = r / M;
  return ((int64_t)i * N + j) * N + k;
}

// global id of edge e of the cell whose lowest grid point is `base`: 3 lin(lower end) + axis
__device__ __forceinline__ int64_t mc_edge_id(int e, int64_t base, int64_t N) {
  const int64_t p = base + nudf_mc_edge[e][0] * N * N + nudf_mc_edge[e][1] * N + nudf_mc_edge[e][2];
  return 3 * p + nudf_mc_edge[e][3];
}

// an edge id taken apart: its lower end p with index triple idx, and its axis
__device__ __forceinline__ void mc_decode_edge(int64_t eid, int64_t N, int64_t& p, int& axis, int64_t (&idx)[3]) {
  p = eid / 3;
  axis = (int)(eid - 3 * p);
  idx[0] = p / (N * N), idx[1] = (p / N) % N, idx[2] = p % N;
}

// is that an edge of the grid at all (a decode that also returned this test made the compiler keep idx in LDS)
__device__ __forceinline__ bool mc_edge_in_grid(int64_t eid, int64_t p, int64_t N, int axis, const int64_t (&idx)[3]) {
  return eid >= 0 && p < N * N * N && idx[axis] < N - 1;
}

// the vertex at weight w from the lower end (index triple idx) of an edge along `axis`; NaN where there is no vertex
__device__ __forceinline__ void mc_store_vertex(float* v, const float* axes, int64_t N, const int64_t (&idx)[3], int axis,
                                                float w) {
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const float xa = axes[x * N + idx[x]];
    v[x] = x == axis ? meshudf_vertex_coord(xa, axes[x * N + idx[x] + 1], w) : xa;
  }
}

__device__ __forceinline__ void mc_store_no_vertex(float* v) { v[0] = v[1] = v[2] = __int_as_float(0x7fc00000); }

// ---- bricks ------------------------------------------------------------------------------------------------------------

// the case index of global cell `cell` (read from its brick) and its lowest grid point; false when the cell is outside
// the grid or its block is not selected
template <class A>
__device__ __forceinline__ bool mc_brick_cell(const A& a, int64_t cell, uint32_t& cs, int64_t& base) {
  const int64_t N = a.N, M = N - 1, B = a.B, nb = a.nb;
  if (cell < 0 || cell >= M * M * M) return false;
  const int64_t k = cell % M, j = (cell / M) % M, i = cell / (M * M);
  const int64_t bi = i / B, bj = j / B, bk = k / B;
  const int64_t slot = a.block_slot[(bi * nb + bj) * nb + bk];
  if (slot < 0 || slot >= a.n_blocks) return false;
  cs = a.cell_case[slot * (B * B * B) + ((i - bi * B) * B + (j - bj * B)) * B + (k - bk * B)];
  base = (i * N + j) * N + k;
  return true;
}

// the brick (-1: none) and block b of the first of the up to 4 cells around a grid edge (lower end idx, along `axis`) whose
// block is selected: it holds both ends of the edge
template <class A>
__device__ __forceinline__ int64_t mc_edge_brick(const A& a, const int64_t (&idx)[3], int axis, int64_t (&b)[3]) {
  const int64_t M = (int64_t)a.N - 1, B = a.B, nb = a.nb;
  const int x1 = (axis + 1) % 3, x2 = (axis + 2) % 3;
  int64_t slot = -1;
  b[axis] = idx[axis] / B;
  for (int d = 0; d < 4 && slot < 0; ++d) {
    const int64_t c1 = idx[x1] - (d >> 1), c2 = idx[x2] - (d & 1);
    if (c1 < 0 || c1 >= M || c2 < 0 || c2 >= M) continue;
    b[x1] = c1 / B;
    b[x2] = c2 / B;
    const int64_t s = a.block_slot[(b[0] * nb + b[1]) * nb + b[2]];
    if (s >= 0 && s < a.n_blocks) slot = s;
  }
  return slot;
}

// first position of the ascending `edges` with edges[pos] >= key
__device__ __forceinline__ int64_t mc_lower_bound(const int64_t* edges, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (edges[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- dense kernels -----------------------------------------------------------------------------------------------------

template <class Rule, class A>
__global__ __launch_bounds__(MC_BLOCK) void mc_dense_classify_kernel(A a) {
  const uint32_t M = (uint32_t)a.N - 1;
  const uint64_t cell = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (cell >= (uint64_t)M * M * M) return;
  const int64_t N = a.N;
  const int64_t base = mc_cell_base((uint32_t)cell, M, N);
  float u[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) u[c] = mc_field(a)[base + mc_corner_offset(c, N)];
  uint32_t nt;
  const uint32_t cs = Rule(a).cell_case(u, [&](int c) { return base + mc_corner_offset(c, N); }, nt);
  if (nt) {
#pragma unroll
    for (int e = 0; e < 12; ++e)
      if (meshudf_edge_crossed(cs, e)) a.edge_flag[mc_edge_id(e, base, N)] = 1;   // every writer stores the same 1
  }
  a.cell_case[cell] = (uint8_t)cs;
  a.cell_ntri[cell] = (uint8_t)nt;
}

template <class A>
__global__ __launch_bounds__(MC_BLOCK) void mc_dense_emit_kernel(A a) {
  const uint64_t t = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  const uint32_t M = (uint32_t)a.N - 1;
  const int64_t cell = a.cells[t];
  if (cell < 0 || cell >= (int64_t)M * M * M) return;
  const int64_t N = a.N;
  const int64_t base = mc_cell_base((uint32_t)cell, M, N);
  const uint32_t cs = a.cell_case[cell];
  const int nt = nudf_mc_ntri[cs];
  const int64_t off = a.face_off[t];
  if (off < 0 || off + nt > a.n_faces) return;
  int64_t* out = a.faces + 3 * off;
  for (int q = 0; q < 3 * nt; ++q) out[q] = a.edge_scan[mc_edge_id(nudf_mc_tri[cs][q], base, N)] - 1;
}

template <class Rule, class A>
__global__ __launch_bounds__(MC_BLOCK) void mc_dense_vertices_kernel(A a) {
  const uint64_t t = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_edges) return;
  const int64_t N = a.N;
  float* v = a.verts + 3 * t;
  int64_t p, idx[3];
  int axis;
  const int64_t eid = a.edges[t];
  mc_decode_edge(eid, N, p, axis, idx);
  if (!mc_edge_in_grid(eid, p, N, axis, idx)) return mc_store_no_vertex(v);
  const int64_t step = axis == 0 ? N * N : (axis == 1 ? N : 1);
  mc_store_vertex(v, a.axes, N, idx, axis, Rule(a).weight(mc_field(a)[p], mc_field(a)[p + step]));
}

// ---- sparse kernels ----------------------------------------------------------------------------------------------------

template <class Rule, int B, class A>
__global__ __launch_bounds__(B == 8 ? 256 : 64) void mc_sparse_classify_kernel(A a) {
  constexpr int P1 = B + 1, P = P1 * P1 * P1, C = B * B * B, T = B == 8 ? 256 : 64;
  __shared__ float su[P];
  const int64_t brick = blockIdx.x;
  if (brick >= a.n_blocks) return;
  for (int t = threadIdx.x; t < P; t += T) su[t] = mc_field(a)[brick * P + t];
  __syncthreads();
  const int64_t nb = a.nb, M = (int64_t)a.N - 1;
  const int64_t blk = a.blocks[brick];
  const bool known = blk >= 0 && blk < nb * nb * nb;
  const int64_t c0[3] = {(blk / (nb * nb)) * B, ((blk / nb) % nb) * B, (blk % nb) * B};   // lowest cell of the block
  for (int lc = threadIdx.x; lc < C; lc += T) {
    const int cz = lc % B, cy = (lc / B) % B, cx = lc / (B * B);
    uint32_t cs = 0, nt = 0;
    if (known && c0[0] + cx < M && c0[1] + cy < M && c0[2] + cz < M) {       // cells past the grid's end emit nothing
      const int base = (cx * P1 + cy) * P1 + cz;
      float u[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) u[c] = su[base + mc_corner_offset(c, P1)];
      cs = Rule(a, brick * P).cell_case(u, [&](int c) { return base + mc_corner_offset(c, P1); }, nt);
    }
    a.cell_case[brick * C + lc] = (uint8_t)cs;
    a.cell_ntri[brick * C + lc] = (uint8_t)nt;
  }
}

template <class A>
__global__ __launch_bounds__(MC_BLOCK) void mc_sparse_edges_kernel(A a) {
  const uint64_t t = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  uint32_t cs = 0;
  int64_t base = 0;
  const bool ok = mc_brick_cell(a, a.cells[t], cs, base) && nudf_mc_ntri[cs];
  int64_t* out = a.edge_keys + 12 * t;
#pragma unroll
  for (int e = 0; e < 12; ++e) out[e] = ok && meshudf_edge_crossed(cs, e) ? mc_edge_id(e, base, a.N) : INT64_MAX;
}

template <class A>
__global__ __launch_bounds__(MC_BLOCK) void mc_sparse_emit_kernel(A a) {
  const uint64_t t = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  uint32_t cs = 0;
  int64_t base = 0;
  if (!mc_brick_cell(a, a.cells[t], cs, base)) return;
  const int nt = nudf_mc_ntri[cs];
  const int64_t off = a.face_off[t];
  if (off < 0 || off + nt > a.n_faces) return;
  int64_t* out = a.faces + 3 * off;
  for (int q = 0; q < 3 * nt; ++q) {
    const int64_t key = mc_edge_id(nudf_mc_tri[cs][q], base, a.N);
    const int64_t lo = mc_lower_bound(a.edges, a.n_edges, key);
    out[q] = lo < a.n_edges && a.edges[lo] == key ? lo : -1;
  }
}

template <class Rule, class A>
__global__ __launch_bounds__(MC_BLOCK) void mc_sparse_vertices_kernel(A a) {
  const uint64_t t = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_edges) return;
  const int64_t N = a.N, M = N - 1, B = a.B, nb = a.nb, P1 = B + 1;
  float* v = a.verts + 3 * t;
  int64_t p, idx[3], slot = -1, b[3] = {0, 0, 0};
  int axis;
  const int64_t eid = a.edges[t];
  mc_decode_edge(eid, N, p, axis, idx);
  if (mc_edge_in_grid(eid, p, N, axis, idx)) slot = mc_edge_brick(a, idx, axis, b);
  if (slot < 0) return mc_store_no_vertex(v);          // not an edge of a selected block
  const int64_t local = ((idx[0] - b[0] * B) * P1 + (idx[1] - b[1] * B)) * P1 + (idx[2] - b[2] * B);
  const int64_t step = axis == 0 ? P1 * P1 : (axis == 1 ? P1 : 1);
  const float* u = mc_field(a) + slot * (P1 * P1 * P1);
  mc_store_vertex(v, a.axes, N, idx, axis, Rule(a).weight(u[local], u[local + step]));
}

// ---- host wrappers -----------------------------------------------------------------------------------------------------

static inline int mc_invalid(const char* where) {
  nudf_set_error(where, hipErrorInvalidValue);
  return (int)hipErrorInvalidValue;
}

template <class A>
static int mc_check_dense(const A& a, const char* where) {
  return a.N >= MC_MIN_N && a.N <= MC_DENSE_MAX_N ? 0 : mc_invalid(where);
}

template <class A>
static int mc_check_sparse(const A& a, const char* where) {
  const bool ok = a.N >= MC_MIN_N && a.N <= MC_SPARSE_MAX_N && (a.B == 4 || a.B == 8) && a.nb == (a.N - 1 + a.B - 1) / a.B &&
                  a.n_blocks >= 0 && a.n_blocks <= (int64_t)a.nb * a.nb * a.nb;
  return ok ? 0 : mc_invalid(where);
}

// `count` work items, `per_group` of them per workgroup of `threads` threads; nothing to do for a count of 0
template <class A>
static int mc_launch(void (*kernel)(A), int64_t count, int per_group, int threads, const A& a, void* stream,
                     const char* name) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((count + per_group - 1) / per_group)), dim3(threads), 0, (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH(name);
  return 0;
}

template <class A>
static int64_t mc_dense_cells(const A& a) { return ((int64_t)a.N - 1) * (a.N - 1) * (a.N - 1); }

// the entry points: `count` work items (an expression over the argument struct `a`) of the kernel, one per thread
#define MC_DENSE_ENTRY(name, Args, count, ...)                                                  \
  extern "C" int name(const Args* args, void* stream) {                                         \
    const Args& a = *args;                                                                      \
    if (int rc = mc_check_dense(a, #name ": N outside [3, 1024]")) return rc;                   \
    return mc_launch(__VA_ARGS__, count, MC_BLOCK, MC_BLOCK, a, stream, #name);                 \
  }

#define MC_SPARSE_WHAT ": N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"
#define MC_SPARSE_ENTRY(name, Args, count, ...)                                                 \
  extern "C" int name(const Args* args, void* stream) {                                         \
    const Args& a = *args;                                                                      \
    if (int rc = mc_check_sparse(a, #name MC_SPARSE_WHAT)) return rc;                           \
    return mc_launch(__VA_ARGS__, count, MC_BLOCK, MC_BLOCK, a, stream, #name);                 \
  }

// sparse classify: one workgroup per brick, 256 threads for B = 8 and 64 for B = 4
#define MC_SPARSE_CLASSIFY_ENTRY(name, Args, Rule)                                              \
  extern "C" int name(const Args* args, void* stream) {                                         \
    const Args& a = *args;                                                                      \
    if (int rc = mc_check_sparse(a, #name MC_SPARSE_WHAT)) return rc;                           \
    return a.B == 8 ? mc_launch(mc_sparse_classify_kernel<Rule, 8, Args>, a.n_blocks, 1, 256, a, stream, #name) \
                    : mc_launch(mc_sparse_classify_kernel<Rule, 4, Args>, a.n_blocks, 1, 64, a, stream, #name); \
  }
