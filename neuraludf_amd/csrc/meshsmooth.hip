// Mesh smoothing and denoising (include/nudf.h NudfMeshOrient sm_ fields, neuraludf_amd/meshclean.py smooth_mesh /
// denoise_mesh): the filters the reference's users leave the GPU for after its mesher (trimesh.smoothing.filter_taubin,
// open3d's filter_smooth_taubin; the reference itself smooths the border only, extract_mesh.py:238-265).
//   laplace -- one thread per vertex: one Jacobi step pos_out = pos + step (m - pos), m the mean of the one-ring in list
//              order (uniform) or the cotangent-weighted mean over the vertex's corners in corner order;
//   frames  -- one thread per face: unit normal, area and centre of the face;
//   normals -- one thread per face: one step of the bilateral normal filter over the faces that share a vertex with it,
//              found through the corner lists of its three vertices taken in ascending vertex index; a face met before,
//              through a vertex visited earlier, is skipped, so every neighbour counts once and in an order that does not
//              depend on the winding; a neighbour's normal is turned into the half-space of the face's own first (the
//              mesher's faces are not consistently wound);
//   update  -- one thread per vertex: one Jacobi step towards the planes of the filtered normals through the centres of
//              the vertex's faces.
// Every thread writes its own item only and sums in list order: no atomics, identical from run to run.  The float64
// expressions follow the numpy restatement (tests/meshsmooth_ref.py) operation by operation: products and sums go through
// mul / add / sub of f64_exact.h under the pragma; the one library call is the exp of the bilateral weight.
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define SM_BLOCK 256

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return add(add(mul(ax, bx), mul(ay, by)), mul(az, bz));
}

__device__ __forceinline__ bool in_range(const NudfMeshOrient& a, const int64_t* t) {
  return t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[0] < a.n_verts && t[1] < a.n_verts && t[2] < a.n_verts;
}

// the corners [b, e) of vertex v, clamped to the list
__device__ __forceinline__ void corner_range(const NudfMeshOrient& a, int64_t v, int64_t* b, int64_t* e) {
  const int64_t n_he = 3 * a.n_faces;
  *b = a.corner_off[v];
  *e = a.corner_off[v + 1];
  if (*b < 0) *b = 0;
  if (*e > n_he) *e = n_he;
}

// cot of the angle at c between x - c and y - c; false where the cross product's length is 0 or not finite
__device__ __forceinline__ bool cotangent(const double* c, const double* x, const double* y, double* cot) {
  const double ux = sub(x[0], c[0]), uy = sub(x[1], c[1]), uz = sub(x[2], c[2]);
  const double vx = sub(y[0], c[0]), vy = sub(y[1], c[1]), vz = sub(y[2], c[2]);
  const double nx = sub(mul(uy, vz), mul(uz, vy)), ny = sub(mul(uz, vx), mul(ux, vz)), nz = sub(mul(ux, vy), mul(uy, vx));
  const double len = __dsqrt_rn(dot3(nx, ny, nz, nx, ny, nz));
  if (!positive_finite(len)) return false;
  *cot = __ddiv_rn(dot3(ux, uy, uz, vx, vy, vz), len);
  return true;
}

__device__ __forceinline__ void copy3(double* o, const double* p) {
  o[0] = p[0];
  o[1] = p[1];
  o[2] = p[2];
}

// ---- (a) one Laplacian step --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_BLOCK) void sm_laplace_kernel(NudfMeshOrient a) {
  const int64_t v = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  const double* p = a.pos + 3 * v;
  double* o = a.sm_pos_out + 3 * v;
  copy3(o, p);
  if (a.sm_fixed && a.sm_fixed[v]) return;
  double sx = 0.0, sy = 0.0, sz = 0.0, W = 0.0;
  if (a.sm_weights == 0) {
    int64_t b = a.sm_nbr_off[v], e = a.sm_nbr_off[v + 1];
    if (b < 0) b = 0;
    if (e > a.sm_n_nbr) e = a.sm_n_nbr;
    int64_t count = 0;
    for (int64_t j = b; j < e; ++j) {
      const int64_t w = a.sm_nbr[j];
      if (w < 0 || w >= a.n_verts) continue;
      const double* q = a.pos + 3 * w;
      sx = add(sx, q[0]);
      sy = add(sy, q[1]);
      sz = add(sz, q[2]);
      ++count;
    }
    W = (double)count;
  } else {
    const int64_t n_he = 3 * a.n_faces;
    int64_t b, e;
    corner_range(a, v, &b, &e);
    for (int64_t j = b; j < e; ++j) {
      const int64_t h = a.corner[j];
      if (h < 0 || h >= n_he) continue;
      const int64_t* t = a.faces + h / 3 * 3;
      if (!in_range(a, t)) continue;
      const int k = (int)(h % 3);
      const double* pc = a.pos + 3 * t[k];             // the corner, the next (a) and the previous (b) vertex of the face
      const double* pa = a.pos + 3 * t[(k + 1) % 3];
      const double* pb = a.pos + 3 * t[(k + 2) % 3];
      double cot_b, cot_a;                             // each angle between the edges to its own next and previous vertex
      if (!cotangent(pb, pc, pa, &cot_b) || !cotangent(pa, pb, pc, &cot_a)) continue;
      const double wa = mul(0.5, cot_b > 0.0 ? cot_b : 0.0), wb = mul(0.5, cot_a > 0.0 ? cot_a : 0.0);
      sx = add(add(sx, mul(wa, pa[0])), mul(wb, pb[0]));
      sy = add(add(sy, mul(wa, pa[1])), mul(wb, pb[1]));
      sz = add(add(sz, mul(wa, pa[2])), mul(wb, pb[2]));
      W = add(W, add(wa, wb));
    }
  }
  if (!positive_finite(W)) return;
  o[0] = add(p[0], mul(a.sm_step, sub(__ddiv_rn(sx, W), p[0])));
  o[1] = add(p[1], mul(a.sm_step, sub(__ddiv_rn(sy, W), p[1])));
  o[2] = add(p[2], mul(a.sm_step, sub(__ddiv_rn(sz, W), p[2])));
}

// ---- (b) face frames ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_BLOCK) void sm_frames_kernel(NudfMeshOrient a) {
  const int64_t f = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  const int64_t* t = a.faces + 3 * f;
  double* on = a.sm_fnormal_out + 3 * f;
  double* oc = a.sm_fcentre + 3 * f;
  on[0] = on[1] = on[2] = 0.0;
  oc[0] = oc[1] = oc[2] = 0.0;
  a.sm_farea[f] = 0.0;
  if (!in_range(a, t)) return;
  const double *p0 = a.pos + 3 * t[0], *p1 = a.pos + 3 * t[1], *p2 = a.pos + 3 * t[2];
  const double ux = sub(p1[0], p0[0]), uy = sub(p1[1], p0[1]), uz = sub(p1[2], p0[2]);
  const double vx = sub(p2[0], p0[0]), vy = sub(p2[1], p0[1]), vz = sub(p2[2], p0[2]);
  const double nx = sub(mul(uy, vz), mul(uz, vy)), ny = sub(mul(uz, vx), mul(ux, vz)), nz = sub(mul(ux, vy), mul(uy, vx));
  const double len = __dsqrt_rn(dot3(nx, ny, nz, nx, ny, nz));
  if (positive_finite(len)) {
    on[0] = __ddiv_rn(nx, len);
    on[1] = __ddiv_rn(ny, len);
    on[2] = __ddiv_rn(nz, len);
  }
  a.sm_farea[f] = mul(0.5, len);
  oc[0] = __ddiv_rn(add(p0[0], add(p1[0], p2[0])), 3.0);
  oc[1] = __ddiv_rn(add(p0[1], add(p1[1], p2[1])), 3.0);
  oc[2] = __ddiv_rn(add(p0[2], add(p1[2], p2[2])), 3.0);
}

// ---- (c) one bilateral step on the face normals --------------------------------------------------------------------------
__device__ __forceinline__ bool has_vertex(const int64_t* t, int64_t v) { return t[0] == v || t[1] == v || t[2] == v; }

__global__ __launch_bounds__(SM_BLOCK) void sm_normals_kernel(NudfMeshOrient a) {
  const int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  if (i >= a.n_faces) return;
  const double* ni = a.sm_fnormal + 3 * i;
  double* o = a.sm_fnormal_out + 3 * i;
  copy3(o, ni);
  const int64_t* t = a.faces + 3 * i;
  if ((ni[0] == 0.0 && ni[1] == 0.0 && ni[2] == 0.0) || !in_range(a, t)) return;
  int64_t u[3] = {t[0], t[1], t[2]};                  // the three vertices in ascending index
  if (u[0] > u[1]) { const int64_t s = u[0]; u[0] = u[1]; u[1] = s; }
  if (u[1] > u[2]) { const int64_t s = u[1]; u[1] = u[2]; u[2] = s; }
  if (u[0] > u[1]) { const int64_t s = u[0]; u[0] = u[1]; u[1] = s; }
  const int64_t n_he = 3 * a.n_faces;
  const double* ci = a.sm_fcentre + 3 * i;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int q = 0; q < 3; ++q) {
    int64_t b, e;
    corner_range(a, u[q], &b, &e);
    for (int64_t j = b; j < e; ++j) {
      const int64_t h = a.corner[j];
      if (h < 0 || h >= n_he) continue;
      const int64_t f = h / 3;
      if (f == i) continue;
      const double* nj = a.sm_fnormal + 3 * f;
      if (nj[0] == 0.0 && nj[1] == 0.0 && nj[2] == 0.0) continue;
      const int64_t* tj = a.faces + 3 * f;
      if ((q > 0 && has_vertex(tj, u[0])) || (q > 1 && has_vertex(tj, u[1]))) continue;     // met through an earlier vertex
      const bool same = dot3(ni[0], ni[1], ni[2], nj[0], nj[1], nj[2]) >= 0.0;
      const double mx = same ? nj[0] : -nj[0], my = same ? nj[1] : -nj[1], mz = same ? nj[2] : -nj[2];
      const double* cj = a.sm_fcentre + 3 * f;
      const double cx = sub(ci[0], cj[0]), cy = sub(ci[1], cj[1]), cz = sub(ci[2], cj[2]);
      const double dx = sub(ni[0], mx), dy = sub(ni[1], my), dz = sub(ni[2], mz);
      const double arg = add(mul(dot3(cx, cy, cz, cx, cy, cz), a.sm_inv2sc), mul(dot3(dx, dy, dz, dx, dy, dz), a.sm_inv2ss));
      const double w = mul(a.sm_farea[f], exp(-arg));
      sx = add(sx, mul(w, mx));
      sy = add(sy, mul(w, my));
      sz = add(sz, mul(w, mz));
    }
  }
  const double len = __dsqrt_rn(dot3(sx, sy, sz, sx, sy, sz));
  if (!positive_finite(len)) return;
  o[0] = __ddiv_rn(sx, len);
  o[1] = __ddiv_rn(sy, len);
  o[2] = __ddiv_rn(sz, len);
}

// ---- (d) one vertex step towards the filtered normals' planes ------------------------------------------------------------
__global__ __launch_bounds__(SM_BLOCK) void sm_update_kernel(NudfMeshOrient a) {
  const int64_t v = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  const double* p = a.pos + 3 * v;
  double* o = a.sm_pos_out + 3 * v;
  copy3(o, p);
  if (a.sm_fixed && a.sm_fixed[v]) return;
  const int64_t n_he = 3 * a.n_faces;
  int64_t b, e;
  corner_range(a, v, &b, &e);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int64_t count = 0;
  for (int64_t j = b; j < e; ++j) {
    const int64_t h = a.corner[j];
    if (h < 0 || h >= n_he) continue;
    const int64_t f = h / 3;
    const double* n = a.sm_fnormal + 3 * f;
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) continue;
    const int64_t* t = a.faces + 3 * f;
    if (!in_range(a, t)) continue;
    const double *p0 = a.pos + 3 * t[0], *p1 = a.pos + 3 * t[1], *p2 = a.pos + 3 * t[2];
    const double dx = sub(__ddiv_rn(add(p0[0], add(p1[0], p2[0])), 3.0), p[0]);
    const double dy = sub(__ddiv_rn(add(p0[1], add(p1[1], p2[1])), 3.0), p[1]);
    const double dz = sub(__ddiv_rn(add(p0[2], add(p1[2], p2[2])), 3.0), p[2]);
    const double d = dot3(n[0], n[1], n[2], dx, dy, dz);
    sx = add(sx, mul(n[0], d));
    sy = add(sy, mul(n[1], d));
    sz = add(sz, mul(n[2], d));
    ++count;
  }
  if (count == 0) return;
  o[0] = add(p[0], __ddiv_rn(sx, (double)count));
  o[1] = add(p[1], __ddiv_rn(sy, (double)count));
  o[2] = add(p[2], __ddiv_rn(sz, (double)count));
}

// ---- launchers --------------------------------------------------------------------------------------------------------
static bool sizes_ok(const NudfMeshOrient& a) {
  return a.n_faces >= 0 && a.n_faces < (1LL << 36) && a.n_verts >= 0 && a.n_verts < (1LL << 31) && a.sm_n_nbr >= 0;
}

#define SM_SIZES "bad sizes (n_verts must be < 2^31, n_faces < 2^36, sm_n_nbr >= 0)"

extern "C" int nudf_meshsmooth_laplace(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshsmooth_laplace";
  if (!sizes_ok(a)) return refuse(entry, SM_SIZES);
  if (a.n_verts <= 0) return 0;
  if (a.sm_weights != 0 && a.sm_weights != 1) return refuse(entry, "sm_weights must be 0 (uniform) or 1 (cotangent)");
  if (!(a.sm_step > -HUGE_VAL && a.sm_step < HUGE_VAL)) return refuse(entry, "sm_step must be finite");
  if (!a.pos || !a.sm_pos_out) return refuse(entry, "NULL pos or sm_pos_out");
  if (a.sm_weights == 0 && (!a.sm_nbr_off || (a.sm_n_nbr > 0 && !a.sm_nbr)))
    return refuse(entry, "NULL sm_nbr_off or sm_nbr");
  if (a.sm_weights == 1 && (!a.corner_off || (a.n_faces > 0 && (!a.corner || !a.faces))))
    return refuse(entry, "NULL corner_off, corner or faces");
  MESH_LAUNCH(sm_laplace_kernel, a.n_verts, SM_BLOCK, SM_BLOCK, entry);
}

extern "C" int nudf_meshsmooth_frames(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshsmooth_frames";
  if (!sizes_ok(a)) return refuse(entry, SM_SIZES);
  if (a.n_faces <= 0) return 0;
  if (!a.faces || !a.pos || !a.sm_fnormal_out || !a.sm_farea || !a.sm_fcentre)
    return refuse(entry, "NULL faces, pos, sm_fnormal_out, sm_farea or sm_fcentre");
  MESH_LAUNCH(sm_frames_kernel, a.n_faces, SM_BLOCK, SM_BLOCK, entry);
}

extern "C" int nudf_meshsmooth_normals(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshsmooth_normals";
  if (!sizes_ok(a)) return refuse(entry, SM_SIZES);
  if (a.n_faces <= 0) return 0;
  if (!positive_finite(a.sm_inv2sc) || !positive_finite(a.sm_inv2ss))
    return refuse(entry, "sm_inv2sc and sm_inv2ss (1 / (2 sigma^2)) must be positive and finite");
  if (!a.faces || !a.corner_off || !a.corner || !a.sm_fnormal || !a.sm_fnormal_out || !a.sm_farea || !a.sm_fcentre)
    return refuse(entry, "NULL faces, corner_off, corner, sm_fnormal, sm_fnormal_out, sm_farea or sm_fcentre");
  MESH_LAUNCH(sm_normals_kernel, a.n_faces, SM_BLOCK, SM_BLOCK, entry);
}

extern "C" int nudf_meshsmooth_update(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshsmooth_update";
  if (!sizes_ok(a)) return refuse(entry, SM_SIZES);
  if (a.n_verts <= 0) return 0;
  if (!a.pos || !a.sm_pos_out || !a.corner_off || (a.n_faces > 0 && (!a.corner || !a.faces || !a.sm_fnormal)))
    return refuse(entry, "NULL pos, sm_pos_out, corner_off, corner, faces or sm_fnormal");
  MESH_LAUNCH(sm_update_kernel, a.n_verts, SM_BLOCK, SM_BLOCK, entry);
}
