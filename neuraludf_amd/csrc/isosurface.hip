// Level-set marching cubes of a scalar grid (include/nudf.h NudfIsoSurface, NudfIsoSurfaceSparse): the surface
// {F = level} of a signed or unsigned field, what the reference gets from PyMCubes in extract_geometry.  Corner c of a
// cell is `-` iff F_c < level; a cell with a non-finite corner emits nothing (isosurface_cell.h).  The pipelines and the
// ordering contract are the MeshUDF mesher's (meshudf.hip, meshudf_sparse.hip) over the same generated case table:
//   dense   classify  -- one thread per cell, consecutive threads along k: case index, triangle count, and a 1 stored at
//                        every sign-change edge of a cell that emits triangles;
//           emit      -- one thread per cell with triangles: its faces at the caller's exclusive scan of the counts,
//                        vertex indices from the caller's inclusive scan of the edge flags;
//           vertices  -- one thread per flagged edge;
//   sparse  classify  -- one workgroup per brick, the brick's (B+1)^3 values staged in LDS;
//           edges     -- one thread per cell with triangles: the global ids of its sign-change edges, INT64_MAX for the
//                        others; the caller sorts and uniques them;
//           emit      -- the vertex of an edge = the position of its id in the sorted unique edge array (binary search);
//           vertices  -- one thread per unique edge: the end values come from a selected brick that holds both ends.
// Every output position is a function of the inputs alone (no atomics).  Dense cell indices fit 32 bits ((N-1)^3 < 2^30
// for N <= 1024); grid point, edge and sparse cell ids are 64-bit (3 N^3 = 2^37.6 at N = 4096).
#include <climits>
#include "nudf_common.h"
#include "../../include/nudf.h"
#include "mc_tables.inc"
#include "isosurface_cell.h"

#define ISO_BLOCK 256
#define ISO_MIN_N 3
#define ISO_MAX_N 1024
#define ISO_SPARSE_MAX_N 4096

// global id of edge e of the cell whose lowest grid point is `base`
__device__ __forceinline__ int64_t iso_edge_id(int e, int64_t base, int64_t N) {
  const int64_t p = base + nudf_mc_edge[e][0] * N * N + nudf_mc_edge[e][1] * N + nudf_mc_edge[e][2];
  return 3 * p + nudf_mc_edge[e][3];
}

// the vertex of edge `eid` with end values fa (lower end, grid index idx) and fb
__device__ __forceinline__ void iso_store_vertex(float* v, const float* axes, int64_t N, const int64_t (&idx)[3], int axis,
                                                 float fa, float fb, float level) {
  const float w = iso_vertex_weight(fa, fb, level);
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const float xa = axes[x * N + idx[x]];
    v[x] = x == axis ? meshudf_vertex_coord(xa, axes[x * N + idx[x] + 1], w) : xa;
  }
}

// ---- dense -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int64_t iso_cell_base(uint32_t cell, uint32_t M, int64_t N) {
  const uint32_t k = cell % M, r = cell / M;
  const uint32_t j = r % M, i = r / M;
  return ((int64_t)i * N + j) * N + k;
}

__global__ __launch_bounds__(ISO_BLOCK) void isosurface_classify_kernel(NudfIsoSurface a) {
  const uint32_t M = (uint32_t)a.N - 1;
  const uint64_t cell = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (cell >= (uint64_t)M * M * M) return;
  const int64_t N = a.N;
  const int64_t base = iso_cell_base((uint32_t)cell, M, N);
  float f[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) f[c] = a.F[base + ((c >> 2) & 1) * N * N + ((c >> 1) & 1) * N + (c & 1)];
  uint32_t nt;
  const uint32_t cs = iso_cell_case(f, a.level, nt);
  if (nt) {
#pragma unroll
    for (int e = 0; e < 12; ++e)
      if (meshudf_edge_crossed(cs, e)) a.edge_flag[iso_edge_id(e, base, N)] = 1;   // every writer stores the same 1
  }
  a.cell_case[cell] = (uint8_t)cs;
  a.cell_ntri[cell] = (uint8_t)nt;
}

__global__ __launch_bounds__(ISO_BLOCK) void isosurface_emit_kernel(NudfIsoSurface a) {
  const uint64_t t = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  const uint32_t M = (uint32_t)a.N - 1;
  const int64_t cell = a.cells[t];
  if (cell < 0 || cell >= (int64_t)M * M * M) return;
  const int64_t N = a.N;
  const int64_t base = iso_cell_base((uint32_t)cell, M, N);
  const uint32_t cs = a.cell_case[cell];
  const int nt = nudf_mc_ntri[cs];
  const int64_t off = a.face_off[t];
  if (off < 0 || off + nt > a.n_faces) return;
  int64_t* out = a.faces + 3 * off;
  for (int q = 0; q < 3 * nt; ++q) out[q] = a.edge_scan[iso_edge_id(nudf_mc_tri[cs][q], base, N)] - 1;
}

__global__ __launch_bounds__(ISO_BLOCK) void isosurface_vertices_kernel(NudfIsoSurface a) {
  const uint64_t t = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_edges) return;
  const int64_t N = a.N;
  const int64_t eid = a.edges[t];
  float* v = a.verts + 3 * t;
  const int64_t p = eid / 3;
  const int axis = (int)(eid - 3 * p);
  const int64_t idx[3] = {p / (N * N), (p / N) % N, p % N};
  if (eid < 0 || p >= N * N * N || idx[axis] >= N - 1) {        // not an edge of the grid: no vertex
    v[0] = v[1] = v[2] = __int_as_float(0x7fc00000);
    return;
  }
  const int64_t step = axis == 0 ? N * N : (axis == 1 ? N : 1);
  iso_store_vertex(v, a.axes, N, idx, axis, a.F[p], a.F[p + step], a.level);
}

static int iso_check_n(const NudfIsoSurface& a, const char* where) {
  if (a.N < ISO_MIN_N || a.N > ISO_MAX_N) {
    nudf_set_error(where, hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

static unsigned iso_blocks(uint64_t n) { return (unsigned)((n + ISO_BLOCK - 1) / ISO_BLOCK); }

extern "C" int nudf_isosurface_struct_size(void) { return (int)sizeof(NudfIsoSurface); }

extern "C" int nudf_isosurface_classify(const NudfIsoSurface* args, void* stream) {
  const NudfIsoSurface& a = *args;
  if (int rc = iso_check_n(a, "nudf_isosurface_classify: N outside [3, 1024]")) return rc;
  const uint64_t M = (uint64_t)a.N - 1;
  hipLaunchKernelGGL(isosurface_classify_kernel, dim3(iso_blocks(M * M * M)), dim3(ISO_BLOCK), 0, (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_classify");
  return 0;
}

extern "C" int nudf_isosurface_emit(const NudfIsoSurface* args, void* stream) {
  const NudfIsoSurface& a = *args;
  if (int rc = iso_check_n(a, "nudf_isosurface_emit: N outside [3, 1024]")) return rc;
  if (a.n_cells <= 0) return 0;
  hipLaunchKernelGGL(isosurface_emit_kernel, dim3(iso_blocks((uint64_t)a.n_cells)), dim3(ISO_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_emit");
  return 0;
}

extern "C" int nudf_isosurface_vertices(const NudfIsoSurface* args, void* stream) {
  const NudfIsoSurface& a = *args;
  if (int rc = iso_check_n(a, "nudf_isosurface_vertices: N outside [3, 1024]")) return rc;
  if (a.n_edges <= 0) return 0;
  hipLaunchKernelGGL(isosurface_vertices_kernel, dim3(iso_blocks((uint64_t)a.n_edges)), dim3(ISO_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_vertices");
  return 0;
}

// ---- sparse ------------------------------------------------------------------------------------------------------------

template <int B>
__global__ __launch_bounds__(B == 8 ? 256 : 64) void isosurface_sparse_classify_kernel(NudfIsoSurfaceSparse a) {
  constexpr int P1 = B + 1, P = P1 * P1 * P1, C = B * B * B, T = B == 8 ? 256 : 64;
  __shared__ float sf[P];
  const int64_t brick = blockIdx.x;
  if (brick >= a.n_blocks) return;
  for (int t = threadIdx.x; t < P; t += T) sf[t] = a.F[brick * P + t];
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
      float f[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) f[c] = sf[base + ((c >> 2) & 1) * P1 * P1 + ((c >> 1) & 1) * P1 + (c & 1)];
      cs = iso_cell_case(f, a.level, nt);
    }
    a.cell_case[brick * C + lc] = (uint8_t)cs;
    a.cell_ntri[brick * C + lc] = (uint8_t)nt;
  }
}

// the case index of global cell `cell` (read from its brick) and its lowest grid point; false when the cell is outside
// the grid or its block is not selected
__device__ __forceinline__ bool iso_sparse_cell(const NudfIsoSurfaceSparse& a, int64_t cell, uint32_t& cs, int64_t& base) {
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

__global__ __launch_bounds__(ISO_BLOCK) void isosurface_sparse_edges_kernel(NudfIsoSurfaceSparse a) {
  const uint64_t t = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  uint32_t cs = 0;
  int64_t base = 0;
  const bool ok = iso_sparse_cell(a, a.cells[t], cs, base) && nudf_mc_ntri[cs];
  int64_t* out = a.edge_keys + 12 * t;
#pragma unroll
  for (int e = 0; e < 12; ++e) out[e] = ok && meshudf_edge_crossed(cs, e) ? iso_edge_id(e, base, a.N) : INT64_MAX;
}

__global__ __launch_bounds__(ISO_BLOCK) void isosurface_sparse_emit_kernel(NudfIsoSurfaceSparse a) {
  const uint64_t t = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  uint32_t cs = 0;
  int64_t base = 0;
  if (!iso_sparse_cell(a, a.cells[t], cs, base)) return;
  const int nt = nudf_mc_ntri[cs];
  const int64_t off = a.face_off[t];
  if (off < 0 || off + nt > a.n_faces) return;
  int64_t* out = a.faces + 3 * off;
  for (int q = 0; q < 3 * nt; ++q) {
    const int64_t key = iso_edge_id(nudf_mc_tri[cs][q], base, a.N);
    int64_t lo = 0, hi = a.n_edges;                    // first position with edges[pos] >= key
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (a.edges[mid] < key) lo = mid + 1; else hi = mid;
    }
    out[q] = lo < a.n_edges && a.edges[lo] == key ? lo : -1;
  }
}

__global__ __launch_bounds__(ISO_BLOCK) void isosurface_sparse_vertices_kernel(NudfIsoSurfaceSparse a) {
  const uint64_t t = (uint64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_edges) return;
  const int64_t N = a.N, M = N - 1, B = a.B, nb = a.nb, P1 = B + 1;
  const int64_t eid = a.edges[t];
  float* v = a.verts + 3 * t;
  const int64_t p = eid / 3;
  const int axis = (int)(eid - 3 * p);
  const int64_t idx[3] = {p / (N * N), (p / N) % N, p % N};
  int64_t slot = -1, b[3] = {0, 0, 0};
  if (eid >= 0 && p < N * N * N && idx[axis] < M) {
    // the up to 4 cells around the edge: the first whose block is selected holds both ends in its brick
    const int x1 = (axis + 1) % 3, x2 = (axis + 2) % 3;
    b[axis] = idx[axis] / B;
    for (int d = 0; d < 4 && slot < 0; ++d) {
      const int64_t c1 = idx[x1] - (d >> 1), c2 = idx[x2] - (d & 1);
      if (c1 < 0 || c1 >= M || c2 < 0 || c2 >= M) continue;
      b[x1] = c1 / B;
      b[x2] = c2 / B;
      const int64_t s = a.block_slot[(b[0] * nb + b[1]) * nb + b[2]];
      if (s >= 0 && s < a.n_blocks) slot = s;
    }
  }
  if (slot < 0) {                                      // not an edge of a selected block: no vertex
    v[0] = v[1] = v[2] = __int_as_float(0x7fc00000);
    return;
  }
  const int64_t local = ((idx[0] - b[0] * B) * P1 + (idx[1] - b[1] * B)) * P1 + (idx[2] - b[2] * B);
  const int64_t step = axis == 0 ? P1 * P1 : (axis == 1 ? P1 : 1);
  const float* f = a.F + slot * (P1 * P1 * P1);
  iso_store_vertex(v, a.axes, N, idx, axis, f[local], f[local + step], a.level);
}

static int iso_sparse_check(const NudfIsoSurfaceSparse& a, const char* where) {
  const bool ok = a.N >= ISO_MIN_N && a.N <= ISO_SPARSE_MAX_N && (a.B == 4 || a.B == 8) &&
                  a.nb == (a.N - 1 + a.B - 1) / a.B && a.n_blocks >= 0 && a.n_blocks <= (int64_t)a.nb * a.nb * a.nb;
  if (!ok) {
    nudf_set_error(where, hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

extern "C" int nudf_isosurface_sparse_struct_size(void) { return (int)sizeof(NudfIsoSurfaceSparse); }

extern "C" int nudf_isosurface_sparse_classify(const NudfIsoSurfaceSparse* args, void* stream) {
  const NudfIsoSurfaceSparse& a = *args;
  if (int rc = iso_sparse_check(a, "nudf_isosurface_sparse_classify: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_blocks == 0) return 0;
  if (a.B == 8)
    hipLaunchKernelGGL(isosurface_sparse_classify_kernel<8>, dim3((unsigned)a.n_blocks), dim3(256), 0, (hipStream_t)stream,
                       a);
  else
    hipLaunchKernelGGL(isosurface_sparse_classify_kernel<4>, dim3((unsigned)a.n_blocks), dim3(64), 0, (hipStream_t)stream,
                       a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_sparse_classify");
  return 0;
}

extern "C" int nudf_isosurface_sparse_edges(const NudfIsoSurfaceSparse* args, void* stream) {
  const NudfIsoSurfaceSparse& a = *args;
  if (int rc = iso_sparse_check(a, "nudf_isosurface_sparse_edges: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_cells <= 0) return 0;
  hipLaunchKernelGGL(isosurface_sparse_edges_kernel, dim3(iso_blocks((uint64_t)a.n_cells)), dim3(ISO_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_sparse_edges");
  return 0;
}

extern "C" int nudf_isosurface_sparse_emit(const NudfIsoSurfaceSparse* args, void* stream) {
  const NudfIsoSurfaceSparse& a = *args;
  if (int rc = iso_sparse_check(a, "nudf_isosurface_sparse_emit: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_cells <= 0) return 0;
  hipLaunchKernelGGL(isosurface_sparse_emit_kernel, dim3(iso_blocks((uint64_t)a.n_cells)), dim3(ISO_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_sparse_emit");
  return 0;
}

extern "C" int nudf_isosurface_sparse_vertices(const NudfIsoSurfaceSparse* args, void* stream) {
  const NudfIsoSurfaceSparse& a = *args;
  if (int rc = iso_sparse_check(a, "nudf_isosurface_sparse_vertices: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_edges <= 0) return 0;
  hipLaunchKernelGGL(isosurface_sparse_vertices_kernel, dim3(iso_blocks((uint64_t)a.n_edges)), dim3(ISO_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_isosurface_sparse_vertices");
  return 0;
}
