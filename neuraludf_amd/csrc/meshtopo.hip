// Mesh topology for the mesh clean-up (include/nudf.h NudfMeshTopo, neuraludf_amd/meshclean.py): what the reference does
// with trimesh / networkx / scipy.sparse / cv2 on the CPU after its mesher (extract_mesh.py:222-265) and before the DTU
// evaluation (evaluation/clean_dtu_mesh.py).
//   edges      -- one thread per unique undirected edge of the key-sorted half-edges: (u, v, count, first face, second
//                 face) and, per half-edge, the row of its edge;
//   fill_count -- one thread per boundary vertex: the number of triangles (0, 1, 2) the hole it is the smallest vertex of
//                 receives;
//   fill_emit  -- the same walk, writing the triangles at the caller's exclusive scan of the counts;
//   smooth     -- one thread per border vertex: one Jacobi step of the border Laplacian, float64, neighbours summed in
//                 ascending vertex index from the previous iteration's positions;
//   cc_hook    -- one thread per sorted half-edge: links the roots of two faces that share the edge (atomicMin; the fixed
//                 point -- label = smallest face index of the component -- does not depend on the order);
//   cc_jump    -- one thread per face: points the face at its root;
//   views      -- one thread per vertex: the number of views whose mask the vertex projects into.
// A key is looked up in the sorted table of unique edge keys by bisection: the row depends on the key alone.  No kernel
// waits on another workgroup.  The float64 expressions follow the numpy restatement (tests/meshclean_ref.py) operation by
// operation; hipcc would fuse a multiply and an add by default, so they go through mul / add / sub of f64_exact.h under
// the pragma (tests/test_meshclean_asm.py).
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define MT_BLOCK 256
#define MT_MAX_LOOP 4

// ---- (a) edge table --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_edges_kernel(NudfMeshTopo a) {
  const int64_t e = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (e >= a.n_edges) return;
  const int64_t n_he = 3 * a.n_faces;
  const int64_t b = a.edge_start[e];
  int64_t end = e + 1 < a.n_edges ? a.edge_start[e + 1] : n_he;
  if (b < 0 || b >= n_he) return;
  end = end > n_he ? n_he : end;
  const int64_t key = a.he_key[b];
  int64_t* row = a.edges + 5 * e;
  row[0] = key / a.n_verts;
  row[1] = key % a.n_verts;
  row[2] = end - b;
  int64_t f0 = -1, f1 = -1;
  for (int64_t j = b; j < end; ++j) {
    const int64_t h = a.he_id[j];                 // ascending within an edge: the sort is stable
    if (h < 0 || h >= n_he) continue;
    if (j == b) f0 = h / 3;
    else if (j == b + 1) f1 = h / 3;
    a.he_edge[h] = e;
  }
  row[3] = f0;
  row[4] = f1;
}

// row of the undirected edge (u, v) in the table, or -1
__device__ int64_t edge_row(const NudfMeshTopo& a, int64_t u, int64_t v) {
  const int64_t key = (u < v ? u : v) * a.n_verts + (u < v ? v : u);
  int64_t lo = 0, hi = a.n_edges;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a.edge_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.n_edges && a.edge_key[lo] == key ? lo : -1;
}

// ---- (b) hole filling (extract_mesh.py:222-223, trimesh fill_holes) -----------------------------------------------------
__device__ __forceinline__ int64_t bdeg(const NudfMeshTopo& a, int64_t v) { return a.nbr_off[v + 1] - a.nbr_off[v]; }

// the hole whose smallest vertex is `v0`: its length (3 or 4) and vertices in walking order, starting towards the
// smaller neighbour; 0 when v0 is not the smallest vertex of a closed loop of <= max_loop boundary edges whose vertices
// all have boundary degree 2
__device__ int hole_of(const NudfMeshTopo& a, int64_t v0, int64_t* loop) {
  if (v0 < 0 || v0 >= a.n_verts || bdeg(a, v0) != 2) return 0;
  const int max_loop = a.max_loop < MT_MAX_LOOP ? a.max_loop : MT_MAX_LOOP;
  loop[0] = v0;
  int64_t prev = v0, cur = a.nbr[a.nbr_off[v0]];
  int len = 1;
  for (;;) {
    if (cur <= v0 || cur >= a.n_verts || bdeg(a, cur) != 2) return 0;
    if (len == max_loop) return 0;
    loop[len++] = cur;
    const int64_t n0 = a.nbr[a.nbr_off[cur]], n1 = a.nbr[a.nbr_off[cur] + 1];
    const int64_t next = n0 == prev ? n1 : n0;
    if (next == v0) break;
    prev = cur;
    cur = next;
  }
  return len >= 3 ? len : 0;
}

__device__ bool face_has(const int64_t* f, int64_t v) { return f[0] == v || f[1] == v || f[2] == v; }

// number of triangles the hole gets: a 3-loop whose triangle already exists gets none
__device__ int hole_triangles(const NudfMeshTopo& a, const int64_t* loop, int len) {
  if (len == 4) return 2;
  if (len != 3) return 0;
  const int64_t e = edge_row(a, loop[0], loop[1]);
  if (e < 0) return 0;
  const int64_t f = a.edges[5 * e + 3];
  if (f >= 0 && f < a.n_faces && face_has(a.faces + 3 * f, loop[2])) return 0;
  return 1;
}

// +1: the face of boundary edge {p, q} runs q -> p (against p -> q); -1: it runs p -> q; 0: not a boundary edge
__device__ int edge_vote(const NudfMeshTopo& a, int64_t p, int64_t q) {
  const int64_t e = edge_row(a, p, q);
  if (e < 0 || a.edges[5 * e + 2] != 1) return 0;
  const int64_t f = a.edges[5 * e + 3];
  if (f < 0 || f >= a.n_faces) return 0;
  const int64_t* t = a.faces + 3 * f;
  for (int k = 0; k < 3; ++k) {
    const int64_t x = t[k], y = t[(k + 1) % 3];
    if (x == p && y == q) return -1;
    if (x == q && y == p) return 1;
  }
  return 0;
}

// writes the triangle {x, y, z} starting at its smallest vertex, ascending unless more of its boundary edges vote for the
// other orientation
__device__ void emit_triangle(const NudfMeshTopo& a, int64_t x, int64_t y, int64_t z, int64_t* out) {
  int64_t t;
  if (x > y) { t = x; x = y; y = t; }
  if (y > z) { t = y; y = z; z = t; }
  if (x > y) { t = x; x = y; y = t; }
  const int vote = edge_vote(a, x, y) + edge_vote(a, y, z) + edge_vote(a, z, x);
  out[0] = x;
  out[1] = vote < 0 ? z : y;
  out[2] = vote < 0 ? y : z;
}

__device__ double dist2(const double* p, const double* q) {
  const double dx = sub(p[0], q[0]), dy = sub(p[1], q[1]), dz = sub(p[2], q[2]);
  return add(add(mul(dx, dx), mul(dy, dy)), mul(dz, dz));
}

__global__ __launch_bounds__(MT_BLOCK) void mt_fill_count_kernel(NudfMeshTopo a) {
  const int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= a.n_bverts) return;
  int64_t loop[MT_MAX_LOOP];
  const int len = hole_of(a, a.bverts[i], loop);
  a.new_count[i] = hole_triangles(a, loop, len);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_fill_emit_kernel(NudfMeshTopo a) {
  const int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= a.n_bverts) return;
  int64_t loop[MT_MAX_LOOP];
  const int len = hole_of(a, a.bverts[i], loop);
  const int n = hole_triangles(a, loop, len);
  const int64_t row = a.new_off[i];
  if (n == 0 || row < 0 || row + n > a.n_new) return;
  int64_t* out = a.new_faces + 3 * row;
  if (n == 1) {
    emit_triangle(a, loop[0], loop[1], loop[2], out);
    return;
  }
  const double* p = a.pos;
  const double dac = dist2(p + 3 * loop[0], p + 3 * loop[2]), dbd = dist2(p + 3 * loop[1], p + 3 * loop[3]);
  if (dac <= dbd) {                              // tie: the diagonal through the smallest index
    emit_triangle(a, loop[0], loop[1], loop[2], out);
    emit_triangle(a, loop[0], loop[2], loop[3], out + 3);
  } else {
    emit_triangle(a, loop[0], loop[1], loop[3], out);
    emit_triangle(a, loop[1], loop[2], loop[3], out + 3);
  }
}

// ---- (c) border smoothing (extract_mesh.py:238-265) ---------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_smooth_kernel(NudfMeshTopo a) {
  const int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= a.n_bverts) return;
  const int64_t v = a.bverts[i];
  if (v < 0 || v >= a.n_verts) return;
  const int64_t b = a.nbr_off[v], e = a.nbr_off[v + 1];
  if (e <= b) return;
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t j = b; j < e; ++j) {
    const int64_t w = a.nbr[j];
    if (w < 0 || w >= a.n_verts) return;
    const double* q = a.pos + 3 * w;
#pragma unroll
    for (int x = 0; x < 3; ++x) s[x] = add(s[x], q[x]);
  }
  const double n = (double)(e - b);
  const double* p = a.pos + 3 * v;
  double* o = a.pos_out + 3 * v;
#pragma unroll
  for (int x = 0; x < 3; ++x) o[x] = add(p[x], mul(a.lam, sub(__ddiv_rn(s[x], n), p[x])));
}

// ---- (d) connected components over faces (clean_dtu_mesh.py:158-191) ---------------------------------------------------
__device__ __forceinline__ int64_t cc_root(const int64_t* labels, int64_t f) {
  for (;;) {                                     // a label is always <= its index: the walk descends and ends at a root
    const int64_t l = __atomic_load_n(labels + f, __ATOMIC_RELAXED);
    if (l == f) return f;
    f = l;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void mt_cc_hook_kernel(NudfMeshTopo a) {
  const int64_t j = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x + 1;
  const int64_t n_he = 3 * a.n_faces;
  if (j >= n_he || a.he_key[j] != a.he_key[j - 1]) return;
  const int64_t ha = a.he_id[j - 1], hb = a.he_id[j];
  if (ha < 0 || hb < 0 || ha >= n_he || hb >= n_he) return;
  const int64_t ra = cc_root(a.labels, ha / 3), rb = cc_root(a.labels, hb / 3);
  if (ra == rb) return;
  const int64_t lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
  atomicMin((unsigned long long*)(a.labels + hi), (unsigned long long)lo);
  *a.changed = 1;
}

__global__ __launch_bounds__(MT_BLOCK) void mt_cc_jump_kernel(NudfMeshTopo a) {
  const int64_t f = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  const int64_t r = cc_root(a.labels, f);
  if (r != f) __atomic_store_n(a.labels + f, r, __ATOMIC_RELAXED);
}

// ---- (e) view cleaning (clean_dtu_mesh.py:36-105) -------------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_views_kernel(NudfMeshTopo a) {
  const int64_t v = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  const double x = a.pos[3 * v], y = a.pos[3 * v + 1], z = a.pos[3 * v + 2];
  const double x_lo = (double)a.border, x_hi = (double)(a.W - a.border);
  const double y_lo = (double)a.border, y_hi = (double)(a.H - a.border);
  int32_t count = 0;
  for (int32_t i = 0; i < a.n_views; ++i) {
    const double* P = a.proj + 12 * i;
    const double qx = add(add(add(mul(P[0], x), mul(P[1], y)), mul(P[2], z)), P[3]);
    const double qy = add(add(add(mul(P[4], x), mul(P[5], y)), mul(P[6], z)), P[7]);
    const double qz = add(add(add(mul(P[8], x), mul(P[9], y)), mul(P[10], z)), P[11]);
    const double u = __ddiv_rn(qx, qz), w = __ddiv_rn(qy, qz);
    if (!(fabs(u) < 0x1p52 && fabs(w) < 0x1p52)) continue;       // non-finite (or far outside any image): counts for nothing
    const double px = add(rint(u), 1.0), py = add(rint(w), 1.0); // rint: half to even, as np.round
    if (!(px >= x_lo && px <= x_hi && py >= y_lo && py <= y_hi)) continue;
    const int32_t ix = (int32_t)px, iy = (int32_t)py;            // 0 <= ix <= W, 0 <= iy <= H
    // the mask padded by one pixel of ones: row 0 and column 0 are padding (W + 1 and H + 1 are outside the window)
    if (ix == 0 || iy == 0 || a.masks[((int64_t)i * a.H + (iy - 1)) * a.W + (ix - 1)]) ++count;
  }
  a.vis_count[v] = count;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
static bool sizes_ok(const NudfMeshTopo& a) {
  return a.n_faces >= 0 && a.n_verts >= 0 && a.n_verts < (1LL << 31) && a.n_faces < (1LL << 40);
}

extern "C" int nudf_meshtopo_edges(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_edges";
  if (!sizes_ok(a) || a.n_edges > 3 * a.n_faces) return refuse(entry, "bad sizes (n_verts must be < 2^31)");
  if (a.n_edges <= 0) return 0;
  if (a.n_verts <= 0) return refuse(entry, "edges without vertices");
  MESH_LAUNCH(mt_edges_kernel, a.n_edges, MT_BLOCK, MT_BLOCK, entry);
}

extern "C" int nudf_meshtopo_fill_count(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_fill_count";
  if (!sizes_ok(a) || a.max_loop < 3 || a.max_loop > MT_MAX_LOOP) return refuse(entry, "max_loop not 3 or 4");
  if (a.n_bverts <= 0) return 0;
  MESH_LAUNCH(mt_fill_count_kernel, a.n_bverts, MT_BLOCK, MT_BLOCK, entry);
}

extern "C" int nudf_meshtopo_fill_emit(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_fill_emit";
  if (!sizes_ok(a) || a.max_loop < 3 || a.max_loop > MT_MAX_LOOP) return refuse(entry, "max_loop not 3 or 4");
  if (a.n_bverts <= 0 || a.n_new <= 0) return 0;
  MESH_LAUNCH(mt_fill_emit_kernel, a.n_bverts, MT_BLOCK, MT_BLOCK, entry);
}

extern "C" int nudf_meshtopo_smooth(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_smooth";
  if (!sizes_ok(a)) return refuse(entry, "bad sizes");
  if (a.n_bverts <= 0) return 0;
  MESH_LAUNCH(mt_smooth_kernel, a.n_bverts, MT_BLOCK, MT_BLOCK, entry);
}

extern "C" int nudf_meshtopo_cc_hook(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_cc_hook";
  if (!sizes_ok(a)) return refuse(entry, "bad sizes");
  if (3 * a.n_faces <= 1) return 0;
  MESH_LAUNCH(mt_cc_hook_kernel, 3 * a.n_faces - 1, MT_BLOCK, MT_BLOCK, entry);
}

extern "C" int nudf_meshtopo_cc_jump(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_cc_jump";
  if (!sizes_ok(a)) return refuse(entry, "bad sizes");
  if (a.n_faces <= 0) return 0;
  MESH_LAUNCH(mt_cc_jump_kernel, a.n_faces, MT_BLOCK, MT_BLOCK, entry);
}

extern "C" int nudf_meshtopo_views(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshtopo_views";
  if (!sizes_ok(a) || a.n_views < 0 || a.H < 1 || a.W < 1 || a.border < 0) return refuse(entry, "bad sizes");
  if (a.n_verts <= 0) return 0;
  MESH_LAUNCH(mt_views_kernel, a.n_verts, MT_BLOCK, MT_BLOCK, entry);
}
