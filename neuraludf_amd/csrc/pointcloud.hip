// Point-cloud geometry of the Chamfer evaluation (include/nudf.h NudfPointCloud): what the reference's
// evaluation/eval_dtu_python.py and eval_deepfashion_python.py do with numpy loops and sklearn KD-trees on the CPU.
//   tri_count  -- one thread per triangle: the float64 quantities of sample_single_tri and the triangle's point count;
//   tri_emit   -- one thread per triangle: its points, in the reference's (i outer, j inner) order, at the caller's
//                 exclusive scan of the counts;
//   keys       -- one thread per point: the cell key floor((p - origin) / cell), 21 bits per axis;
//   cells      -- one thread per occupied cell: inserts key -> row of the sorted cell table into an open-addressing hash
//                 (64-bit atomicCAS on the key; the row depends only on the key, not on the order of insertion);
//   thin_round -- one thread per undecided point (cell-sorted): the greedy radius thinning as rounds of a
//                 lexicographically-first maximal independent set in rank order;
//   nearest    -- one thread per query (cell-sorted): exact nearest neighbour by Chebyshev rings of cells, up to `bound`.
// Every float64 expression is evaluated in the reference's (numpy's / sklearn's) operation order with no contraction:
// products and sums go through mul / add / sub of f64_exact.h, plain operators under the pragma
// (tests/test_pointcloud_asm.py).  The cell key, the hash and the ring walk are those of cell_index.h, which meshdist.hip
// and meshray.hip search the same table with.
#pragma clang fp contract(off)

#include "cell_index.h"
#include "mesh_launch.h"

#define PC_BLOCK 256
#define PC_UNDECIDED 0
#define PC_KEEP 1
#define PC_DROP 2

__device__ __forceinline__ double dist2(const double* p, double qx, double qy, double qz) {
  return dot3(sub(qx, p[0]), sub(qy, p[1]), sub(qz, p[2]));
}

// ---- mesh sampling (eval_dtu_python.py:225-258, sample_single_tri :21-30) -------------------------------------------
struct Tri {
  double t0[3], v1[3], v2[3];
  double n1, n2, d1, d2;          // n = floor(l / thr); d = max(n, 1e-7) (Python's max: n unless 1e-7 > n)
};

// false: a triangle the reference drops (area2 > 0 fails, NaN included) or a face index out of range
__device__ bool tri_setup(const NudfPointCloud& a, int64_t f, Tri& t) {
  const int64_t* fi = a.faces + 3 * f;
  const int64_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.n_verts || i1 >= a.n_verts || i2 >= a.n_verts) return false;
  const double *p0 = a.verts + 3 * i0, *p1 = a.verts + 3 * i1, *p2 = a.verts + 3 * i2;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    t.t0[x] = p0[x];
    t.v1[x] = sub(p1[x], p0[x]);
    t.v2[x] = sub(p2[x], p0[x]);
  }
  const double l1 = __dsqrt_rn(dot3(t.v1[0], t.v1[1], t.v1[2]));
  const double l2 = __dsqrt_rn(dot3(t.v2[0], t.v2[1], t.v2[2]));
  const double cx = sub(mul(t.v1[1], t.v2[2]), mul(t.v1[2], t.v2[1]));   // np.cross order
  const double cy = sub(mul(t.v1[2], t.v2[0]), mul(t.v1[0], t.v2[2]));
  const double cz = sub(mul(t.v1[0], t.v2[1]), mul(t.v1[1], t.v2[0]));
  const double area2 = __dsqrt_rn(dot3(cx, cy, cz));
  if (!(area2 > 0.0)) return false;
  const double thr = mul(a.density, __dsqrt_rn(__ddiv_rn(mul(l1, l2), area2)));
  t.n1 = floor(__ddiv_rn(l1, thr));
  t.n2 = floor(__ddiv_rn(l2, thr));
  t.d1 = 1e-7 > t.n1 ? 1e-7 : t.n1;
  t.d2 = 1e-7 > t.n2 ? 1e-7 : t.n2;
  return true;
}

// number of j in [0, n2] with c0 + (j + .5) / d2 < 1: a prefix of j, since the rounded sum is monotone in j
__device__ int64_t row_count(const Tri& t, double c0) {
  int64_t lo = 0, hi = (int64_t)t.n2 + 1;     // invariant: j < lo passes, j >= hi fails
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (add(c0, __ddiv_rn(add((double)mid, 0.5), t.d2)) < 1.0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(PC_BLOCK) void pc_tri_count_kernel(NudfPointCloud a) {
  const int64_t f = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  Tri t;
  int64_t n = 0;
  if (tri_setup(a, f, t)) {
    if (!(t.n1 >= 1.0 && t.n2 >= 1.0)) {
      n = (t.n1 >= 0.0 && t.n2 >= 0.0) ? 0 : a.cap + 1;    // n = 0 on an axis: every c >= 0.5 / 1e-7; NaN: refused
    } else if (t.n1 * t.n2 > 4.0 * (double)a.cap) {
      n = a.cap + 1;                                        // at least ~n1 n2 / 2 points: over the cap for sure
    } else {
      for (int64_t i = 0; i <= (int64_t)t.n1 && n <= a.cap; ++i) {
        const int64_t r = row_count(t, __ddiv_rn(add((double)i, 0.5), t.d1));
        if (r == 0) break;                                  // c0 grows with i: no later row has a point either
        n += r;
      }
      if (n > a.cap) n = a.cap + 1;
    }
  }
  a.tri_n[f] = n;
}

__global__ __launch_bounds__(PC_BLOCK) void pc_tri_emit_kernel(NudfPointCloud a) {
  const int64_t f = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  const int64_t n = a.tri_n[f];
  if (n <= 0 || n > a.cap) return;
  Tri t;
  if (!tri_setup(a, f, t)) return;
  int64_t row = a.out_base + a.tri_off[f];
  const int64_t end = row + n;
  if (row < 0 || end > a.n_out) return;
  for (int64_t i = 0; i <= (int64_t)t.n1 && row < end; ++i) {
    const double c0 = __ddiv_rn(add((double)i, 0.5), t.d1);
    for (int64_t j = 0; j <= (int64_t)t.n2 && row < end; ++j) {
      const double c1 = __ddiv_rn(add((double)j, 0.5), t.d2);
      if (!(add(c0, c1) < 1.0)) break;
      double* q = a.out + 3 * row++;
#pragma unroll
      for (int x = 0; x < 3; ++x) q[x] = add(add(mul(t.v1[x], c0), mul(t.v2[x], c1)), t.t0[x]);
    }
  }
}

// ---- building the cell index (cell_index.h) ------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLOCK) void pc_keys_kernel(NudfPointCloud a) {
  const int64_t s = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (s >= a.n) return;
  const double* p = a.pts + 3 * s;
  a.keys[s] = pack_key(clamp_axis(cell_coord(p[0], a.origin[0], a.cell)),
                       clamp_axis(cell_coord(p[1], a.origin[1], a.cell)),
                       clamp_axis(cell_coord(p[2], a.origin[2], a.cell)));
}

__global__ __launch_bounds__(PC_BLOCK) void pc_cells_kernel(NudfPointCloud a) {
  const int64_t r = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (r >= a.n_cells) return;
  const int64_t key = a.cell_key[r];
  const uint64_t mask = (uint64_t)a.hash_cap - 1;
  uint64_t h = probe_first(key, mask);                      // the sequence cell_row follows
  for (int64_t probe = 0; probe < a.hash_cap; ++probe) {
    const unsigned long long old =
        atomicCAS((unsigned long long*)(a.hash_key + h), (unsigned long long)PC_EMPTY, (unsigned long long)key);
    if (old == (unsigned long long)PC_EMPTY || old == (unsigned long long)key) {
      a.hash_row[h] = r;
      return;
    }
    h = probe_next(h, mask);
  }
}

// ---- radius thinning (eval_dtu_python.py:265-276) -------------------------------------------------------------------
// Point p (rank = its position after the shuffle) is KEEP iff no lower-ranked KEEP point lies within r of it: the
// reference's sequential loop.  A round decides p as DROP when a lower-ranked neighbour is KEEP, as KEEP when every
// lower-ranked neighbour is DROP; it reads the states in place (a state only moves from UNDECIDED to final, so a value it
// reads is either final or UNDECIDED, and either way the decision is the sequential one).  The lowest-ranked undecided
// point is decided in every round.
__global__ __launch_bounds__(PC_BLOCK) void pc_thin_round_kernel(NudfPointCloud a) {
  const int64_t s = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (s >= a.n || a.state[s] != PC_UNDECIDED) return;
  const double* p = a.pts + 3 * s;
  const double px = p[0], py = p[1], pz = p[2];
  const int64_t rank = a.rank[s], key = a.keys[s];
  const int64_t cx = key >> (2 * PC_AXIS_BITS), cy = (key >> PC_AXIS_BITS) & PC_AXIS_MAX, cz = key & PC_AXIS_MAX;
  bool open = false;
  for (int64_t x = cx - 1; x <= cx + 1; ++x) {
    if (x < 0 || x >= a.grid[0]) continue;
    for (int64_t y = cy - 1; y <= cy + 1; ++y) {
      if (y < 0 || y >= a.grid[1]) continue;
      for (int64_t z = cz - 1; z <= cz + 1; ++z) {
        if (z < 0 || z >= a.grid[2]) continue;
        const int64_t row = cell_row(a, pack_key(x, y, z));
        if (row < 0) continue;
        const int64_t b = a.cell_start[row], e = b + a.cell_count[row];
        for (int64_t t = b; t < e; ++t) {
          if (a.rank[t] >= rank) continue;
          if (!(dist2(a.pts + 3 * t, px, py, pz) <= a.r2)) continue;
          const uint8_t st = __atomic_load_n(a.state + t, __ATOMIC_RELAXED);
          if (st == PC_KEEP) {
            a.state[s] = PC_DROP;
            return;
          }
          if (st == PC_UNDECIDED) open = true;
        }
      }
    }
  }
  if (open) atomicAdd(a.undecided, 1);
  else a.state[s] = PC_KEEP;
}

// ---- nearest neighbour (sklearn kneighbors, n_neighbors=1) --------------------------------------------------------------
// The ring walk of cell_index.h over the points' cells.  Candidates are compared by the reported value sqrt(d2), ties by
// the lower reference index; d2 screens out the rest (two d2 more than 2^-48 apart relative have different square roots).
__global__ __launch_bounds__(PC_BLOCK) void pc_nearest_kernel(NudfPointCloud a) {
  const int64_t t = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
  if (t >= a.n_query) return;
  const double* q = a.query + 3 * t;
  const double qx = q[0], qy = q[1], qz = q[2];
  const int64_t out = a.query_idx[t];
  double best = __longlong_as_double(0x7ff0000000000000LL), best_d2 = best;
  int64_t best_i = -1;
  auto visit = [&](int64_t x, int64_t y, int64_t z) {
    const int64_t row = cell_row(a, pack_key(x, y, z));
    if (row < 0) return;
    const int64_t b = a.cell_start[row], e = b + a.cell_count[row];
    for (int64_t s = b; s < e; ++s) {
      const double d2 = dist2(a.pts + 3 * s, qx, qy, qz);
      if (!(d2 <= mul(best_d2, 1.0 + 0x1p-48))) continue;
      const double d = __dsqrt_rn(d2);
      const int64_t i = a.rank[s];
      if (d < best) {
        best = d;
        best_i = i;
        best_d2 = d2;
      } else if (d == best && i < best_i) {
        best_i = i;
        best_d2 = d2 < best_d2 ? d2 : best_d2;
      }
    }
  };
  ring_walk(a, qx, qy, qz, visit, [&] { return best; });
  if (!(best <= a.bound)) {
    best = __longlong_as_double(0x7ff0000000000000LL);
    best_i = -1;
  }
  a.dist[out] = best;
  a.idx[out] = best_i;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
extern "C" int nudf_pc_tri_count(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_tri_count";
  if (a.n_faces <= 0) return 0;
  if (a.cap < 0 || !(a.density > 0.0)) return refuse(entry, "cap < 0 or density <= 0");
  MESH_LAUNCH(pc_tri_count_kernel, a.n_faces, PC_BLOCK, PC_BLOCK, entry);
}

extern "C" int nudf_pc_tri_emit(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_tri_emit";
  if (a.n_faces <= 0) return 0;
  if (a.cap < 0 || !(a.density > 0.0)) return refuse(entry, "cap < 0 or density <= 0");
  MESH_LAUNCH(pc_tri_emit_kernel, a.n_faces, PC_BLOCK, PC_BLOCK, entry);
}

extern "C" int nudf_pc_keys(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_keys";
  if (a.n <= 0) return 0;
  if (!(a.cell > 0.0)) return refuse(entry, "cell <= 0");
  MESH_LAUNCH(pc_keys_kernel, a.n, PC_BLOCK, PC_BLOCK, entry);
}

extern "C" int nudf_pc_cells(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_cells";
  if (a.n_cells <= 0) return 0;
  if (a.hash_cap < 2 * a.n_cells || (a.hash_cap & (a.hash_cap - 1)))
    return refuse(entry, "hash_cap must be a power of two >= 2 n_cells");
  MESH_LAUNCH(pc_cells_kernel, a.n_cells, PC_BLOCK, PC_BLOCK, entry);
}

extern "C" int nudf_pc_thin_round(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_thin_round";
  if (a.n <= 0) return 0;
  if (!grid_ok(a) || !(a.cell > 0.0) || a.hash_cap < 2) return refuse(entry, "bad grid, cell or hash table");
  MESH_LAUNCH(pc_thin_round_kernel, a.n, PC_BLOCK, PC_BLOCK, entry);
}

extern "C" int nudf_pc_nearest(const NudfPointCloud* args, void* stream) {
  const NudfPointCloud& a = *args;
  const char* const entry = "nudf_pc_nearest";
  if (a.n_query <= 0) return 0;
  if (!grid_ok(a) || !(a.cell > 0.0) || a.hash_cap < 2 || a.n <= 0)
    return refuse(entry, "bad grid, cell or hash table");
  MESH_LAUNCH(pc_nearest_kernel, a.n_query, PC_BLOCK, PC_BLOCK, entry);
}
