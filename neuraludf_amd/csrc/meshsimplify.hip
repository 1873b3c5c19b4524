// Mesh simplification by vertex clustering with quadric placement (include/nudf.h NudfMeshTopo, the sp_ fields;
// neuraludf_amd/meshclean.py simplify_mesh / simplify_to_faces): clusters are the occupied cells of a uniform grid
// (Rossignac-Borrel), each cluster's representative minimises the sum of its faces' plane quadrics (Lindstrom) plus the
// quadrics of the planes that stand on its border edges.  The reference has no counterpart: its users leave the GPU for
// trimesh or open3d at this step.
//   keys   -- one thread per vertex: the cell of the vertex and its int64 key, -1 for a vertex that is not finite or lies
//             outside the grid;
//   place  -- one thread per cluster: one walk over the cluster's corners (ascending 3 f + k) that sums the quadric, one
//             over its member vertices (ascending index) for the mean, the regularised 3 x 3 Cholesky solve, the test that
//             the solution lies in the cluster's own cell, and the attribute means;
//   faces  -- one thread per face: the three cluster ids, whether two of them are equal, and the ids in ascending order
//             for the caller's sort.
// Every sum runs in list order inside one thread: no atomics, the result is identical from run to run.  No kernel waits on
// another workgroup.  The float64 expressions follow the numpy restatement (tests/meshsimplify_ref.py) operation by
// operation: products and sums go through mul / add / sub of f64_exact.h under the pragma.
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define SP_BLOCK 256
#define SP_MAX_GRID (1LL << 20)

__device__ __forceinline__ double dot3(const double* a, const double* b) {
  return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]));
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = sub(mul(a[1], b[2]), mul(a[2], b[1]));
  o[1] = sub(mul(a[2], b[0]), mul(a[0], b[2]));
  o[2] = sub(mul(a[0], b[1]), mul(a[1], b[0]));
}

// ---- (a) keys -----------------------------------------------------------------------------------------------------------
// key = (cx Gy + cy) Gz + cz with c = floor((p - origin) / cell) per axis, or -1 when a coordinate is not finite or its
// cell lies outside [0, G)
__device__ int64_t sp_key_of(const NudfMeshTopo& a, const double* p) {
  int64_t c[3];
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const double q = floor(__ddiv_rn(sub(p[x], a.sp_origin[x]), a.sp_cell));
    if (!(q >= 0.0 && q < (double)a.sp_grid[x])) return -1;        // NaN fails both comparisons
    c[x] = (int64_t)q;
  }
  return (c[0] * a.sp_grid[1] + c[1]) * a.sp_grid[2] + c[2];
}

__global__ __launch_bounds__(SP_BLOCK) void sp_keys_kernel(NudfMeshTopo a) {
  const int64_t v = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  a.sp_key[v] = sp_key_of(a, a.pos + 3 * v);
}

// ---- (b) placement ------------------------------------------------------------------------------------------------------
// adds the plane with unit normal u through point `through`, weight w, to the quadric q = (A00 A01 A02 A11 A12 A22, b, c),
// in coordinates local to `centre`
__device__ __forceinline__ void sp_add_plane(double* q, const double* u, const double* through, const double* centre,
                                             double w) {
  const double r[3] = {sub(through[0], centre[0]), sub(through[1], centre[1]), sub(through[2], centre[2])};
  const double d = -dot3(u, r);
  const double wd = mul(w, d);
  q[0] = add(q[0], mul(w, mul(u[0], u[0])));
  q[1] = add(q[1], mul(w, mul(u[0], u[1])));
  q[2] = add(q[2], mul(w, mul(u[0], u[2])));
  q[3] = add(q[3], mul(w, mul(u[1], u[1])));
  q[4] = add(q[4], mul(w, mul(u[1], u[2])));
  q[5] = add(q[5], mul(w, mul(u[2], u[2])));
  q[6] = add(q[6], mul(wd, u[0]));
  q[7] = add(q[7], mul(wd, u[1]));
  q[8] = add(q[8], mul(wd, u[2]));
  q[9] = add(q[9], mul(wd, d));
}

// half-edge h lies on an edge with exactly one half-edge
__device__ __forceinline__ bool sp_on_border(const NudfMeshTopo& a, int64_t h) {
  const int64_t e = a.he_edge[h];
  return e >= 0 && e < a.n_edges && a.edges[5 * e + 2] == 1;
}

// the boundary plane of half-edge j of the face with corners p[0..2] and unit normal u: through p[j], normal (e x u) / |e x u|
__device__ __forceinline__ void sp_add_border(double* q, const double* const* p, int j, const double* u,
                                              const double* centre, double w) {
  const double* s = p[j];
  const double* t = p[(j + 1) % 3];
  const double e[3] = {sub(t[0], s[0]), sub(t[1], s[1]), sub(t[2], s[2])};
  double m[3];
  cross3(e, u, m);
  const double len = __dsqrt_rn(dot3(m, m));
  if (!positive_finite(len)) return;
  const double mu[3] = {__ddiv_rn(m[0], len), __ddiv_rn(m[1], len), __ddiv_rn(m[2], len)};
  sp_add_plane(q, mu, s, centre, w);
}

__global__ __launch_bounds__(SP_BLOCK) void sp_place_kernel(NudfMeshTopo a) {
  const int64_t c = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
  if (c >= a.n_clusters) return;
  const int64_t key = a.sp_cluster_key[c];
  const int64_t gyz = a.sp_grid[1] * a.sp_grid[2];
  const int64_t cell[3] = {key / gyz, key / a.sp_grid[2] % a.sp_grid[1], key % a.sp_grid[2]};
  double centre[3];
#pragma unroll
  for (int x = 0; x < 3; ++x) centre[x] = add(a.sp_origin[x], mul(add((double)cell[x], 0.5), a.sp_cell));

  // the mean of the members, local to the centre
  int64_t mb = a.sp_member_off[c], me = a.sp_member_off[c + 1];
  if (mb < 0) mb = 0;
  if (me > a.n_verts) me = a.n_verts;
  double mean[3] = {0.0, 0.0, 0.0};
  for (int64_t j = mb; j < me; ++j) {
    const int64_t v = a.sp_member[j];
    if (v < 0 || v >= a.n_verts) continue;
    const double* p = a.pos + 3 * v;
#pragma unroll
    for (int x = 0; x < 3; ++x) mean[x] = add(mean[x], sub(p[x], centre[x]));
  }
  const double count = (double)(me - mb);
#pragma unroll
  for (int x = 0; x < 3; ++x) mean[x] = __ddiv_rn(mean[x], count);

  double rep[3] = {mean[0], mean[1], mean[2]};
  bool accepted = false;
  if (a.sp_placement == 0) {
    const int64_t n_he = 3 * a.n_faces;
    const bool border = a.sp_boundary_weight != 0.0 && a.he_edge != nullptr && a.edges != nullptr;
    int64_t cb = a.sp_corner_off[c], ce = a.sp_corner_off[c + 1];
    if (cb < 0) cb = 0;
    if (ce > n_he) ce = n_he;
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t j = cb; j < ce; ++j) {
      const int64_t h = a.sp_corner[j];
      if (h < 0 || h >= n_he) continue;
      const int64_t f = h / 3;
      const int k = (int)(h % 3);
      const int64_t* t = a.faces + 3 * f;
      const int64_t v0 = t[0], v1 = t[1], v2 = t[2];
      if (v0 < 0 || v1 < 0 || v2 < 0 || v0 >= a.n_verts || v1 >= a.n_verts || v2 >= a.n_verts) continue;
      const double* p[3] = {a.pos + 3 * v0, a.pos + 3 * v1, a.pos + 3 * v2};
      const double e1[3] = {sub(p[1][0], p[0][0]), sub(p[1][1], p[0][1]), sub(p[1][2], p[0][2])};
      const double e2[3] = {sub(p[2][0], p[0][0]), sub(p[2][1], p[0][1]), sub(p[2][2], p[0][2])};
      double n[3];
      cross3(e1, e2, n);
      const double len = __dsqrt_rn(dot3(n, n));
      if (!positive_finite(len)) continue;                  // zero area or not finite: the face adds nothing
      const double u[3] = {__ddiv_rn(n[0], len), __ddiv_rn(n[1], len), __ddiv_rn(n[2], len)};
      const double w = mul(len, 0.5);
      sp_add_plane(q, u, p[0], centre, w);
      if (border) {
        const double wb = mul(a.sp_boundary_weight, w);
        const int into = (k + 2) % 3;                       // the half-edge that ends at this corner
        if (sp_on_border(a, 3 * f + k)) sp_add_border(q, p, k, u, centre, wb);
        if (sp_on_border(a, 3 * f + into)) sp_add_border(q, p, into, u, centre, wb);
      }
    }
    if (a.sp_quadric != nullptr) {
#pragma unroll
      for (int x = 0; x < 10; ++x) a.sp_quadric[10 * c + x] = q[x];
    }
    const double tr = add(add(q[0], q[3]), q[5]);
    if (tr > 0.0) {
      // (A + lam tr I) x = -b + lam tr mean: Cholesky without pivoting (condition <= (1 + lam) / lam)
      const double lt = mul(a.sp_lambda, tr);
      const double m00 = add(q[0], lt), m10 = q[1], m20 = q[2], m11 = add(q[3], lt), m21 = q[4], m22 = add(q[5], lt);
      const double r0 = add(-q[6], mul(lt, mean[0])), r1 = add(-q[7], mul(lt, mean[1])), r2 = add(-q[8], mul(lt, mean[2]));
      const double l00 = __dsqrt_rn(m00);
      const double l10 = __ddiv_rn(m10, l00), l20 = __ddiv_rn(m20, l00);
      const double l11 = __dsqrt_rn(sub(m11, mul(l10, l10)));
      const double l21 = __ddiv_rn(sub(m21, mul(l20, l10)), l11);
      const double l22 = __dsqrt_rn(sub(sub(m22, mul(l20, l20)), mul(l21, l21)));
      const double y0 = __ddiv_rn(r0, l00);
      const double y1 = __ddiv_rn(sub(r1, mul(l10, y0)), l11);
      const double y2 = __ddiv_rn(sub(sub(r2, mul(l20, y0)), mul(l21, y1)), l22);
      const double x2 = __ddiv_rn(y2, l22);
      const double x1 = __ddiv_rn(sub(y1, mul(l21, x2)), l11);
      const double x0 = __ddiv_rn(sub(sub(y0, mul(l10, x1)), mul(l20, x2)), l00);
      const double at[3] = {add(centre[0], x0), add(centre[1], x1), add(centre[2], x2)};
      if (sp_key_of(a, at) == key) {                        // a solution that is not finite has key -1
        accepted = true;
        rep[0] = x0;
        rep[1] = x1;
        rep[2] = x2;
      }
    }
  }
#pragma unroll
  for (int x = 0; x < 3; ++x) a.sp_rep[3 * c + x] = add(centre[x], rep[x]);
  a.sp_accepted[c] = accepted ? 1 : 0;

  // attribute means: the members again, one column at a time
  for (int32_t col = 0; col < a.sp_attr_width; ++col) {
    double s = 0.0;
    for (int64_t j = mb; j < me; ++j) {
      const int64_t v = a.sp_member[j];
      if (v < 0 || v >= a.n_verts) continue;
      s = add(s, a.sp_attr[v * a.sp_attr_width + col]);
    }
    a.sp_attr_out[c * a.sp_attr_width + col] = __ddiv_rn(s, count);
  }
}

// ---- (c) faces ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_BLOCK) void sp_faces_kernel(NudfMeshTopo a) {
  const int64_t f = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  int64_t r[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t v = a.faces[3 * f + k];
    const bool in = v >= 0 && v < a.n_verts;
    r[k] = in ? a.sp_vcluster[v] : -1;
    ok = ok && in;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) a.sp_faces[3 * f + k] = r[k];
  a.sp_degenerate[f] = !ok || r[0] == r[1] || r[1] == r[2] || r[0] == r[2];
  int64_t t;
  if (r[0] > r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] > r[2]) { t = r[1]; r[1] = r[2]; r[2] = t; }
  if (r[0] > r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
#pragma unroll
  for (int k = 0; k < 3; ++k) a.sp_triple[3 * f + k] = r[k];
}

// ---- launchers --------------------------------------------------------------------------------------------------------
static bool sizes_ok(const NudfMeshTopo& a) {
  if (!(a.n_faces >= 0 && a.n_verts >= 0 && a.n_verts < (1LL << 31) && a.n_faces < (1LL << 40))) return false;
  if (a.n_clusters < 0 || a.n_clusters > a.n_verts || a.n_edges < 0 || a.n_edges > 3 * a.n_faces) return false;
  for (int x = 0; x < 3; ++x)
    if (a.sp_grid[x] < 0 || a.sp_grid[x] > SP_MAX_GRID) return false;
  return a.sp_attr_width >= 0;
}

// what a launch that computes keys needs besides: a grid and a cell to compute them with
static bool grid_ok(const NudfMeshTopo& a) {
  for (int x = 0; x < 3; ++x)
    if (a.sp_grid[x] < 1 || !(a.sp_origin[x] > -HUGE_VAL && a.sp_origin[x] < HUGE_VAL)) return false;
  return a.sp_cell > 0.0 && a.sp_cell < HUGE_VAL;
}

#define SP_SIZES "bad sizes (n_verts must be < 2^31, a grid dimension <= 2^20, the attribute width >= 0)"
#define SP_GRID "the cell must be positive and finite, the origin finite and every grid dimension >= 1"

extern "C" int nudf_meshsimplify_keys(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsimplify_keys";
  if (!sizes_ok(a)) return refuse(entry, SP_SIZES);
  if (a.n_verts <= 0) return 0;
  if (!grid_ok(a)) return refuse(entry, SP_GRID);
  if (!a.pos || !a.sp_key) return refuse(entry, "pos or sp_key is NULL");
  MESH_LAUNCH(sp_keys_kernel, a.n_verts, SP_BLOCK, SP_BLOCK, entry);
}

extern "C" int nudf_meshsimplify_place(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsimplify_place";
  if (!sizes_ok(a)) return refuse(entry, SP_SIZES);
  if (a.n_clusters <= 0) return 0;
  if (!grid_ok(a)) return refuse(entry, SP_GRID);
  if (a.sp_placement != 0 && a.sp_placement != 1) return refuse(entry, "sp_placement not 0 or 1");
  if (!(a.sp_lambda > 0.0 && a.sp_lambda < HUGE_VAL) || !(a.sp_boundary_weight >= 0.0 && a.sp_boundary_weight < HUGE_VAL))
    return refuse(entry, "sp_lambda must be positive, sp_boundary_weight not negative, both finite");
  if (!a.pos || !a.sp_cluster_key || !a.sp_member_off || !a.sp_member || !a.sp_rep || !a.sp_accepted)
    return refuse(entry, "pos, sp_cluster_key, sp_member_off, sp_member, sp_rep or sp_accepted is NULL");
  if (a.sp_placement == 0 && (!a.faces || !a.sp_corner_off || !a.sp_corner))
    return refuse(entry, "faces, sp_corner_off or sp_corner is NULL");
  if (a.sp_attr_width > 0 && (!a.sp_attr || !a.sp_attr_out))
    return refuse(entry, "sp_attr or sp_attr_out is NULL with sp_attr_width > 0");
  MESH_LAUNCH(sp_place_kernel, a.n_clusters, SP_BLOCK, SP_BLOCK, entry);
}

extern "C" int nudf_meshsimplify_faces(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshsimplify_faces";
  if (!sizes_ok(a)) return refuse(entry, SP_SIZES);
  if (a.n_faces <= 0) return 0;
  if (!a.faces || !a.sp_vcluster || !a.sp_faces || !a.sp_triple || !a.sp_degenerate)
    return refuse(entry, "faces, sp_vcluster, sp_faces, sp_triple or sp_degenerate is NULL");
  MESH_LAUNCH(sp_faces_kernel, a.n_faces, SP_BLOCK, SP_BLOCK, entry);
}
