// Sparse MeshUDF extraction (include/nudf.h NudfMeshUDFSparse): the dense mesher's cells and edges (meshudf.hip, the
// shared arithmetic in meshudf_cell.h) over the bricks of the selected B^3-cell blocks only.
//   classify  -- one workgroup per brick, the brick's (B+1)^3 values staged in LDS (each is a corner of up to 8 cells);
//                G is read from memory in active cells only: case index and triangle count per brick cell;
//   edges     -- one thread per cell with triangles (the caller's ascending list of global cell indices): the global id
//                of each of its sign-change edges, INT64_MAX for the other edges; the caller sorts and uniques them;
//   emit      -- one thread per cell with triangles: its faces at the caller's exclusive scan of the counts, the vertex
//                of an edge = the position of its id in the sorted unique edge array (binary search);
//   vertices  -- one thread per unique edge: the end values come from a selected brick that holds both ends, found
//                through block_slot (every copy of a shared node holds the same bits).
// No dense N^3 array and no atomics: every output position is a function of the inputs alone.
// Global cell, node and edge ids are 64-bit (3 N^3 = 2^37.6 at N = 4096); block ids fit 32 bits (nb <= 1024).
#include <climits>
#include "nudf_common.h"
#include "../../include/nudf.h"
#include "mc_tables.inc"
#include "meshudf_cell.h"

#define MUS_BLOCK 256
#define MUS_MIN_N 3
#define MUS_MAX_N 4096

template <int B>
__global__ __launch_bounds__(B == 8 ? 256 : 64) void meshudf_sparse_classify_kernel(NudfMeshUDFSparse a) {
  constexpr int P1 = B + 1, P = P1 * P1 * P1, C = B * B * B, T = B == 8 ? 256 : 64;
  __shared__ float su[P];
  const int64_t brick = blockIdx.x;
  if (brick >= a.n_blocks) return;
  for (int t = threadIdx.x; t < P; t += T) su[t] = a.U[brick * P + t];
  __syncthreads();
  const int64_t nb = a.nb, M = (int64_t)a.N - 1;
  const int64_t blk = a.blocks[brick];
  const bool known = blk >= 0 && blk < nb * nb * nb;
  const int64_t c0[3] = {(blk / (nb * nb)) * B, ((blk / nb) % nb) * B, (blk % nb) * B};   // lowest cell of the block
  const float* g = a.G + 3 * brick * P;
  for (int lc = threadIdx.x; lc < C; lc += T) {
    const int cz = lc % B, cy = (lc / B) % B, cx = lc / (B * B);
    uint32_t cs = 0, nt = 0;
    if (known && c0[0] + cx < M && c0[1] + cy < M && c0[2] + cz < M) {       // cells past the grid's end emit nothing
      const int base = (cx * P1 + cy) * P1 + cz;
      float u[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) u[c] = su[base + ((c >> 2) & 1) * P1 * P1 + ((c >> 1) & 1) * P1 + (c & 1)];
      cs = meshudf_cell_case(u, a.mean_thr, a.max_thr, [&](int c) {
        return g + 3 * (base + ((c >> 2) & 1) * P1 * P1 + ((c >> 1) & 1) * P1 + (c & 1));
      }, nt);
    }
    a.cell_case[brick * C + lc] = (uint8_t)cs;
    a.cell_ntri[brick * C + lc] = (uint8_t)nt;
  }
}

// the case index of global cell `cell` (read from its brick) and its lowest grid point; false when the cell is outside
// the grid or its block is not selected
__device__ __forceinline__ bool mus_cell(const NudfMeshUDFSparse& a, int64_t cell, uint32_t& cs, int64_t& base) {
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

__device__ __forceinline__ int64_t mus_edge_id(int e, int64_t base, int64_t N) {
  const int64_t p = base + nudf_mc_edge[e][0] * N * N + nudf_mc_edge[e][1] * N + nudf_mc_edge[e][2];
  return 3 * p + nudf_mc_edge[e][3];
}

__global__ __launch_bounds__(MUS_BLOCK) void meshudf_sparse_edges_kernel(NudfMeshUDFSparse a) {
  const uint64_t t = (uint64_t)blockIdx.x * MUS_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  uint32_t cs = 0;
  int64_t base = 0;
  const bool ok = mus_cell(a, a.cells[t], cs, base) && nudf_mc_ntri[cs];
  int64_t* out = a.edge_keys + 12 * t;
#pragma unroll
  for (int e = 0; e < 12; ++e) out[e] = ok && meshudf_edge_crossed(cs, e) ? mus_edge_id(e, base, a.N) : INT64_MAX;
}

__global__ __launch_bounds__(MUS_BLOCK) void meshudf_sparse_emit_kernel(NudfMeshUDFSparse a) {
  const uint64_t t = (uint64_t)blockIdx.x * MUS_BLOCK + threadIdx.x;
  if (t >= (uint64_t)a.n_cells) return;
  uint32_t cs = 0;
  int64_t base = 0;
  if (!mus_cell(a, a.cells[t], cs, base)) return;
  const int nt = nudf_mc_ntri[cs];
  const int64_t off = a.face_off[t];
  if (off < 0 || off + nt > a.n_faces) return;
  int64_t* out = a.faces + 3 * off;
  for (int q = 0; q < 3 * nt; ++q) {
    const int64_t key = mus_edge_id(nudf_mc_tri[cs][q], base, a.N);
    int64_t lo = 0, hi = a.n_edges;                    // first position with edges[pos] >= key
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (a.edges[mid] < key) lo = mid + 1; else hi = mid;
    }
    out[q] = lo < a.n_edges && a.edges[lo] == key ? lo : -1;
  }
}

__global__ __launch_bounds__(MUS_BLOCK) void meshudf_sparse_vertices_kernel(NudfMeshUDFSparse a) {
  const uint64_t t = (uint64_t)blockIdx.x * MUS_BLOCK + threadIdx.x;
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
  const float* u = a.U + slot * (P1 * P1 * P1);
  const float w = meshudf_vertex_weight(u[local], u[local + step]);
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const float xa = a.axes[x * N + idx[x]];
    v[x] = x == axis ? meshudf_vertex_coord(xa, a.axes[x * N + idx[x] + 1], w) : xa;
  }
}

static int check_args(const NudfMeshUDFSparse& a, const char* where) {
  const bool ok = a.N >= MUS_MIN_N && a.N <= MUS_MAX_N && (a.B == 4 || a.B == 8) && a.nb == (a.N - 1 + a.B - 1) / a.B &&
                  a.n_blocks >= 0 && a.n_blocks <= (int64_t)a.nb * a.nb * a.nb;
  if (!ok) {
    nudf_set_error(where, hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

static unsigned blocks_of(uint64_t n) { return (unsigned)((n + MUS_BLOCK - 1) / MUS_BLOCK); }

extern "C" int nudf_meshudf_sparse_struct_size(void) { return (int)sizeof(NudfMeshUDFSparse); }

extern "C" int nudf_meshudf_sparse_classify(const NudfMeshUDFSparse* args, void* stream) {
  const NudfMeshUDFSparse& a = *args;
  if (int rc = check_args(a, "nudf_meshudf_sparse_classify: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_blocks == 0) return 0;
  if (a.B == 8)
    hipLaunchKernelGGL(meshudf_sparse_classify_kernel<8>, dim3((unsigned)a.n_blocks), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(meshudf_sparse_classify_kernel<4>, dim3((unsigned)a.n_blocks), dim3(64), 0, (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_meshudf_sparse_classify");
  return 0;
}

extern "C" int nudf_meshudf_sparse_edges(const NudfMeshUDFSparse* args, void* stream) {
  const NudfMeshUDFSparse& a = *args;
  if (int rc = check_args(a, "nudf_meshudf_sparse_edges: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_cells <= 0) return 0;
  hipLaunchKernelGGL(meshudf_sparse_edges_kernel, dim3(blocks_of((uint64_t)a.n_cells)), dim3(MUS_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_meshudf_sparse_edges");
  return 0;
}

extern "C" int nudf_meshudf_sparse_emit(const NudfMeshUDFSparse* args, void* stream) {
  const NudfMeshUDFSparse& a = *args;
  if (int rc = check_args(a, "nudf_meshudf_sparse_emit: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_cells <= 0) return 0;
  hipLaunchKernelGGL(meshudf_sparse_emit_kernel, dim3(blocks_of((uint64_t)a.n_cells)), dim3(MUS_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_meshudf_sparse_emit");
  return 0;
}

extern "C" int nudf_meshudf_sparse_vertices(const NudfMeshUDFSparse* args, void* stream) {
  const NudfMeshUDFSparse& a = *args;
  if (int rc = check_args(a, "nudf_meshudf_sparse_vertices: N outside [3, 4096], B not 4 or 8, or nb / n_blocks wrong"))
    return rc;
  if (a.n_edges <= 0) return 0;
  hipLaunchKernelGGL(meshudf_sparse_vertices_kernel, dim3(blocks_of((uint64_t)a.n_edges)), dim3(MUS_BLOCK), 0,
                     (hipStream_t)stream, a);
  NUDF_CHECK_LAUNCH("nudf_meshudf_sparse_vertices");
  return 0;
}
