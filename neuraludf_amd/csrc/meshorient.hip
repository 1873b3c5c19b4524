// Consistent face orientation and vertex normals (include/nudf.h NudfMeshOrient, neuraludf_amd/meshclean.py orient_faces /
// vertex_normals): what the reference declines to do after its mesher (extract_mesh.py:218-219, trimesh's serial graph
// traversal) and the trimesh.geometry.weighted_vertex_normals it calls at extract_mesh.py:272-275.
//   hook    -- one thread per manifold edge (two half-edges of two different, non-degenerate faces): a union-find over the
//              faces in which every face holds one packed word, parent * 2 + parity; parity = 1 says that the face and its
//              parent need opposite flips.  The two faces' roots are found with the parities along the walks, and the larger
//              root takes the smaller as parent (64-bit atomicMin of the packed word);
//   jump    -- one thread per face: its own word becomes (root, parity to the root);
//   check   -- one thread per manifold edge, after the rounds: marks the component's label where the two parities
//              contradict the edge (plain stores of 1);
//   outward -- one wavefront per component: S = sum over its faces of N_f . (c_f - origin) with the flips of the words
//              applied, lane l adding the faces l, l + 64, ... of the component in that order and the 64 lane sums added
//              in lane order: a fixed order, no floating-point atomics;
//   normals -- one thread per vertex over its corners in ascending 3 f + k: angle-weighted normals, float64.
// A parent is always smaller than its child, so every walk descends and ends.  Every word ever written states a relation
// that follows from the edges seen so far: in an orientable component all of them agree with its one solution, whatever
// the order in which the atomics land, and in any component the fixed point of the labels is the smallest face index.
// No kernel waits on another workgroup.  The float64 expressions follow the numpy restatement (tests/meshorient_ref.py)
// operation by operation: products and sums go through mul / add / sub of f64_exact.h under the pragma.
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define MO_BLOCK 256
#define MO_WAVE 64

// ---- (a) parity union-find ---------------------------------------------------------------------------------------------
// root of face f and, in `parity`, whether f and the root need opposite flips
__device__ __forceinline__ int64_t mo_find(const int64_t* word, int64_t f, int* parity) {
  int p = 0;
  for (;;) {
    const int64_t w = __atomic_load_n(word + f, __ATOMIC_RELAXED);
    const int64_t parent = w >> 1;
    if (parent < 0 || parent >= f) break;          // a root holds 2 f; anything else that does not descend ends the walk too
    p ^= (int)(w & 1);
    f = parent;
  }
  *parity = p;
  return f;
}

// the two faces of manifold edge e and whether they run along it in the same direction; false when the edge is out of range
__device__ __forceinline__ bool mo_edge(const NudfMeshOrient& a, int64_t e, int64_t* fa, int64_t* fb, int* same) {
  const int64_t n_he = 3 * a.n_faces;
  const int64_t ha = a.me_a[e], hb = a.me_b[e];
  if (ha < 0 || hb < 0 || ha >= n_he || hb >= n_he) return false;
  *fa = ha / 3;
  *fb = hb / 3;
  *same = a.faces[ha] == a.faces[hb];              // half-edge h starts at faces[h]: equal starts = the same direction
  return true;
}

__global__ __launch_bounds__(MO_BLOCK) void mo_hook_kernel(NudfMeshOrient a) {
  const int64_t e = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x;
  if (e >= a.n_medges) return;
  int64_t fa, fb;
  int same, pa, pb;
  if (!mo_edge(a, e, &fa, &fb, &same)) return;
  const int64_t ra = mo_find(a.word, fa, &pa), rb = mo_find(a.word, fb, &pb);
  if (ra == rb) return;
  const int64_t lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
  // flip(fa) ^ flip(fb) = same, flip(f) = flip(root) ^ parity  ->  flip(ra) ^ flip(rb) = pa ^ pb ^ same
  atomicMin((unsigned long long*)(a.word + hi), (unsigned long long)(2 * lo + (pa ^ pb ^ same)));
  *a.changed = 1;
}

__global__ __launch_bounds__(MO_BLOCK) void mo_jump_kernel(NudfMeshOrient a) {
  const int64_t f = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x;
  if (f >= a.n_faces) return;
  int p;
  const int64_t r = mo_find(a.word, f, &p);
  if (r != f) __atomic_store_n(a.word + f, 2 * r + p, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(MO_BLOCK) void mo_check_kernel(NudfMeshOrient a) {
  const int64_t e = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x;
  if (e >= a.n_medges) return;
  int64_t fa, fb;
  int same;
  if (!mo_edge(a, e, &fa, &fb, &same)) return;
  const int64_t wa = a.word[fa], wb = a.word[fb];  // after the last jump: (label, parity to the label)
  const int64_t label = wa >> 1;
  if (label < 0 || label >= a.n_faces) return;
  if (((wa ^ wb) & 1) != same) a.nonorient[label] = 1;
}

// ---- (b) outward sum ---------------------------------------------------------------------------------------------------
// N_f . (c_f - origin) of face f with the flip of its word applied.  c_f = (p0 + (p1 + p2)) / 3: a flip swaps p1 and p2, so
// it negates N_f and keeps c_f bit for bit -- the sum of the complementary set of flips is exactly the negative.
__device__ double mo_outward_term(const NudfMeshOrient& a, int64_t f) {
  const int64_t* t = a.faces + 3 * f;
  const bool flip = a.word[f] & 1;
  const int64_t v0 = t[0], v1 = flip ? t[2] : t[1], v2 = flip ? t[1] : t[2];
  if (v0 < 0 || v1 < 0 || v2 < 0 || v0 >= a.n_verts || v1 >= a.n_verts || v2 >= a.n_verts) return 0.0;
  const double *p0 = a.pos + 3 * v0, *p1 = a.pos + 3 * v1, *p2 = a.pos + 3 * v2;
  const double ux = sub(p1[0], p0[0]), uy = sub(p1[1], p0[1]), uz = sub(p1[2], p0[2]);
  const double vx = sub(p2[0], p0[0]), vy = sub(p2[1], p0[1]), vz = sub(p2[2], p0[2]);
  const double nx = sub(mul(uy, vz), mul(uz, vy)), ny = sub(mul(uz, vx), mul(ux, vz)), nz = sub(mul(ux, vy), mul(uy, vx));
  const double dx = sub(__ddiv_rn(add(p0[0], add(p1[0], p2[0])), 3.0), a.origin[0]);
  const double dy = sub(__ddiv_rn(add(p0[1], add(p1[1], p2[1])), 3.0), a.origin[1]);
  const double dz = sub(__ddiv_rn(add(p0[2], add(p1[2], p2[2])), 3.0), a.origin[2]);
  return add(add(mul(nx, dx), mul(ny, dy)), mul(nz, dz));
}

__global__ __launch_bounds__(MO_BLOCK) void mo_outward_kernel(NudfMeshOrient a) {
  const int64_t c = (int64_t)blockIdx.x * (MO_BLOCK / MO_WAVE) + threadIdx.x / MO_WAVE;
  const int lane = threadIdx.x % MO_WAVE;
  // a whole wavefront shares c: it leaves or stays as one, and the shuffles below see all 64 lanes
  if (c >= a.n_comps) return;
  int64_t b = a.comp_off[c], e = a.comp_off[c + 1];
  if (b < 0) b = 0;
  if (e > a.n_faces) e = a.n_faces;
  double acc = 0.0;
  for (int64_t j = b + lane; j < e; j += MO_WAVE) {
    const int64_t f = a.comp_face[j];
    if (f >= 0 && f < a.n_faces) acc = add(acc, mo_outward_term(a, f));
  }
  double s = 0.0;
  for (int l = 0; l < MO_WAVE; ++l) s = add(s, __shfl(acc, l, MO_WAVE));
  if (lane == 0) a.comp_sum[c] = s;
}

// ---- (c) angle-weighted vertex normals (extract_mesh.py:272-275, trimesh weighted_vertex_normals) ------------------------
__global__ __launch_bounds__(MO_BLOCK) void mo_normals_kernel(NudfMeshOrient a) {
  const int64_t v = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  const int64_t n_he = 3 * a.n_faces;
  int64_t b = a.corner_off[v], e = a.corner_off[v + 1];
  if (b < 0) b = 0;
  if (e > n_he) e = n_he;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t j = b; j < e; ++j) {
    const int64_t h = a.corner[j];
    if (h < 0 || h >= n_he) continue;
    const int64_t* t = a.faces + h / 3 * 3;
    const int k = (int)(h % 3);
    const int64_t v0 = t[0], v1 = t[1], v2 = t[2];
    if (v0 < 0 || v1 < 0 || v2 < 0 || v0 >= a.n_verts || v1 >= a.n_verts || v2 >= a.n_verts) continue;
    const double *p0 = a.pos + 3 * v0, *p1 = a.pos + 3 * v1, *p2 = a.pos + 3 * v2;
    const double ux = sub(p1[0], p0[0]), uy = sub(p1[1], p0[1]), uz = sub(p1[2], p0[2]);
    const double wx = sub(p2[0], p0[0]), wy = sub(p2[1], p0[1]), wz = sub(p2[2], p0[2]);
    const double nx = sub(mul(uy, wz), mul(uz, wy)), ny = sub(mul(uz, wx), mul(ux, wz)), nz = sub(mul(ux, wy), mul(uy, wx));
    const double len = __dsqrt_rn(add(add(mul(nx, nx), mul(ny, ny)), mul(nz, nz)));
    if (!(len > 0.0 && len < HUGE_VAL)) continue;  // zero area or not finite: contributes nothing
    const double* pc = a.pos + 3 * t[k];           // the corner, the next and the previous vertex of the face
    const double* pn = a.pos + 3 * t[(k + 1) % 3];
    const double* pp = a.pos + 3 * t[(k + 2) % 3];
    const double ax = sub(pn[0], pc[0]), ay = sub(pn[1], pc[1]), az = sub(pn[2], pc[2]);
    const double bx = sub(pp[0], pc[0]), by = sub(pp[1], pc[1]), bz = sub(pp[2], pc[2]);
    const double theta = atan2(len, add(add(mul(ax, bx), mul(ay, by)), mul(az, bz)));
    sx = add(sx, mul(theta, __ddiv_rn(nx, len)));
    sy = add(sy, mul(theta, __ddiv_rn(ny, len)));
    sz = add(sz, mul(theta, __ddiv_rn(nz, len)));
  }
  const double len = __dsqrt_rn(add(add(mul(sx, sx), mul(sy, sy)), mul(sz, sz)));
  const bool ok = len > 0.0 && len < HUGE_VAL;
  double* o = a.normals + 3 * v;
  o[0] = ok ? __ddiv_rn(sx, len) : 0.0;
  o[1] = ok ? __ddiv_rn(sy, len) : 0.0;
  o[2] = ok ? __ddiv_rn(sz, len) : 0.0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
static bool sizes_ok(const NudfMeshOrient& a) {
  return a.n_faces >= 0 && a.n_faces < (1LL << 36) && a.n_verts >= 0 && a.n_verts < (1LL << 31) && a.n_medges >= 0 &&
         a.n_medges <= 3 * a.n_faces / 2 && a.n_comps >= 0 && a.n_comps <= a.n_faces;
}

#define MO_SIZES_MEDGES "bad sizes (n_verts must be < 2^31, n_medges <= 3 n_faces / 2)"

extern "C" int nudf_meshorient_hook(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshorient_hook";
  if (!sizes_ok(a)) return refuse(entry, MO_SIZES_MEDGES);
  if (a.n_medges <= 0) return 0;
  MESH_LAUNCH(mo_hook_kernel, a.n_medges, MO_BLOCK, MO_BLOCK, entry);
}

extern "C" int nudf_meshorient_jump(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshorient_jump";
  if (!sizes_ok(a)) return refuse(entry, MO_SIZES_MEDGES);
  if (a.n_faces <= 0) return 0;
  MESH_LAUNCH(mo_jump_kernel, a.n_faces, MO_BLOCK, MO_BLOCK, entry);
}

extern "C" int nudf_meshorient_check(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshorient_check";
  if (!sizes_ok(a)) return refuse(entry, MO_SIZES_MEDGES);
  if (a.n_medges <= 0) return 0;
  MESH_LAUNCH(mo_check_kernel, a.n_medges, MO_BLOCK, MO_BLOCK, entry);
}

extern "C" int nudf_meshorient_outward(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshorient_outward";
  if (!sizes_ok(a)) return refuse(entry, "bad sizes (n_verts must be < 2^31, n_comps <= n_faces)");
  if (a.n_comps <= 0) return 0;
  MESH_LAUNCH(mo_outward_kernel, a.n_comps, MO_BLOCK, MO_BLOCK / MO_WAVE, entry);
}

extern "C" int nudf_meshorient_normals(const NudfMeshOrient* args, void* stream) {
  const NudfMeshOrient& a = *args;
  const char* const entry = "nudf_meshorient_normals";
  if (!sizes_ok(a)) return refuse(entry, "bad sizes (n_verts must be < 2^31)");
  if (a.n_verts <= 0) return 0;
  MESH_LAUNCH(mo_normals_kernel, a.n_verts, MO_BLOCK, MO_BLOCK, entry);
}
