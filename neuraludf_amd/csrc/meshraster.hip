// Triangle rasteriser with a depth buffer (include/nudf.h NudfMeshRaster, neuraludf_amd/meshrender.py): depth, face and
// barycentric maps of a mesh from the dataset cameras, depth-tested vertex visibility, vertex colours from the images.
//   project    -- one thread per (view, vertex): screen coordinates and camera depth, float64;
//   bounds     -- one thread per (view, face): the number of pixels of its clamped box, 0 for a face that draws nothing;
//   draw_small -- one thread per (view, face) of the small list: every pixel of its box (most faces of a 512^3 mesh cover
//                 a pixel or two at 1600 x 1200);
//   draw_large -- one wavefront per (view, face) of the large list, lanes striding the box row-major;
//   resolve    -- one thread per pixel: depth, face and barycentrics from the winning key;
//   visible    -- one thread per (view, vertex): the depth test against the 3 x 3 maximum around its pixel;
//   colour     -- one thread per vertex over the views in ascending order: weighted mean of bilinear samples.
// The depth buffer holds one 64-bit key per pixel, (bits of the float32 depth) << 32 | face: positive floats order as their
// bits, so a 64-bit unsigned atomicMin keeps the nearest face and, among equal depths, the smallest face index -- whatever
// the order in which the atomics land.  No floating-point atomics, no kernel waits on another workgroup.  The float64
// expressions follow the numpy restatement (tests/meshraster_ref.py) operation by operation: products and sums go through
// mul / add / sub of f64_exact.h under the pragma.
#pragma clang fp contract(off)

#include "meshraster_pixel.h"
#include "mesh_launch.h"

#define MR_BLOCK 256
#define MR_WAVE 64

// ---- (a) projection and boxes ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_BLOCK) void mr_project_kernel(NudfMeshRaster a) {
  const int64_t i = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= (int64_t)a.n_views * a.n_verts) return;
  const int64_t view = i / a.n_verts, v = i - view * a.n_verts;
  mr_project(a.proj + 12 * view, a.pos + 3 * v, a.scr + 3 * i);
}

__global__ __launch_bounds__(MR_BLOCK) void mr_bounds_kernel(NudfMeshRaster a) {
  const int64_t i = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= (int64_t)a.n_views * a.n_faces) return;
  const int64_t view = i / a.n_faces, f = i - view * a.n_faces;
  MrFace t;
  mr_face(a, view, f, &t);
  a.npix[i] = t.bw * t.bh;                           // <= H * W < 2^31
}

// ---- (b) drawing -------------------------------------------------------------------------------------------------------
// the (view, face) of entry e; false when the entry is out of range
__device__ __forceinline__ bool mr_entry(const NudfMeshRaster& a, int64_t e, int64_t* view, int64_t* f) {
  const int64_t id = a.entries[e];
  if (id < 0 || id >= (int64_t)a.n_views * a.n_faces) return false;
  *view = id / a.n_faces;
  *f = id - *view * a.n_faces;
  return true;
}

__global__ __launch_bounds__(MR_BLOCK) void mr_draw_small_kernel(NudfMeshRaster a) {
  const int64_t e = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (e >= a.n_entries) return;
  int64_t view, f;
  MrFace t;
  if (!mr_entry(a, e, &view, &f) || !mr_face(a, view, f, &t)) return;
  const int32_t n = t.bw * t.bh;
  for (int32_t i = 0; i < n; ++i) mr_draw(a, t, view, f, i);
}

__global__ __launch_bounds__(MR_BLOCK) void mr_draw_large_kernel(NudfMeshRaster a) {
  const int64_t e = (int64_t)blockIdx.x * (MR_BLOCK / MR_WAVE) + threadIdx.x / MR_WAVE;
  const int lane = threadIdx.x % MR_WAVE;
  if (e >= a.n_entries) return;
  int64_t view, f;
  MrFace t;
  if (!mr_entry(a, e, &view, &f) || !mr_face(a, view, f, &t)) return;
  const int32_t n = t.bw * t.bh;
  for (int32_t i = lane; i < n; i += MR_WAVE) mr_draw(a, t, view, f, i);
}

// ---- (c) resolve -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_BLOCK) void mr_resolve_kernel(NudfMeshRaster a) {
  const int64_t i = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  const int64_t hw = (int64_t)a.H * a.W;
  if (i >= a.n_views * hw) return;
  const unsigned long long key = a.zbuf[i];
  const int64_t f = (int64_t)(key & 0xffffffffULL);
  float depth = HUGE_VALF, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  int32_t face = -1;
  if (key != MR_EMPTY && f < a.n_faces) {
    const int64_t view = i / hw, p = i - view * hw;
    depth = __uint_as_float((unsigned)(key >> 32));
    face = (int32_t)f;
    if (a.bary) {
      MrFace t;
      double b[3], z;
      if (mr_face(a, view, f, &t) && mr_pixel(t, (int32_t)(p % a.W), (int32_t)(p / a.W), b, &z))
        b0 = (float)b[0], b1 = (float)b[1], b2 = (float)b[2];
    }
  }
  a.depth[i] = depth;
  if (a.face) a.face[i] = face;
  if (a.bary) a.bary[3 * i] = b0, a.bary[3 * i + 1] = b1, a.bary[3 * i + 2] = b2;
}

// ---- (d) visibility ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_BLOCK) void mr_visible_kernel(NudfMeshRaster a) {
  const int64_t i = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= (int64_t)a.n_views * a.n_verts) return;
  const int64_t view = i / a.n_verts;
  a.vis[i] = mr_seen(a, view, a.scr + 3 * i);
}

// ---- (e) vertex colours ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_BLOCK) void mr_colour_kernel(NudfMeshRaster a) {
  const int64_t v = (int64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (v >= a.n_verts) return;
  const double* p = a.pos + 3 * v;
  double sw = 0.0, sc[3] = {0.0, 0.0, 0.0};
  int32_t n = 0;
  for (int64_t view = 0; view < a.n_views; ++view) {
    if (!a.vis[view * a.n_verts + v]) continue;
    double s[3];
    mr_project(a.proj + 12 * view, p, s);
    // (vis is the caller's: mr_taps keeps every tap inside the image whatever the projection is, NaN included)
    mr_accumulate(a, view, p, s, a.normals ? a.normals + 3 * v : nullptr, &sw, sc);
    ++n;
  }
  const bool ok = sw > 0.0 && sw < HUGE_VAL;
  for (int c = 0; c < 3; ++c) a.colors[3 * v + c] = ok ? (float)__ddiv_rn(sc[c], sw) : a.fill[c];
  a.n_seen[v] = ok ? n : 0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
#define MR_MAX_THREADS (1LL << 38)                   // one-dimensional grids of MR_BLOCK threads: < 2^31 blocks

static bool sizes_ok(const NudfMeshRaster& a) {
  if (a.n_faces < 0 || a.n_faces >= (1LL << 31) || a.n_verts < 0 || a.n_verts >= (1LL << 31)) return false;
  if (a.n_views < 0 || a.H < 0 || a.W < 0 || a.n_entries < 0) return false;
  if ((int64_t)a.H * a.W >= (1LL << 31)) return false;                   // npix is int32
  if ((int64_t)a.n_views * a.H * a.W > MR_MAX_THREADS) return false;    // n_views < 2^31, H W < 2^31: no overflow
  if (a.n_views * a.n_faces > MR_MAX_THREADS || a.n_views * a.n_verts > MR_MAX_THREADS) return false;
  return a.n_entries <= a.n_views * a.n_faces;
}

#define MR_BAD_SIZES \
  "bad sizes (n_faces, n_verts and H * W must be < 2^31, n_views * H * W, n_views * n_faces and n_views * n_verts " \
  "<= 2^38, n_entries <= n_views * n_faces, nothing negative)"

// an image is needed as soon as there is something to do per view
#define MR_NEED_IMAGE \
  if (a.H < 1 || a.W < 1) return refuse(entry, "H and W must be >= 1")

extern "C" int nudf_meshraster_project(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_project";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_views <= 0 || a.n_verts <= 0) return 0;
  MESH_LAUNCH(mr_project_kernel, a.n_views * a.n_verts, MR_BLOCK, MR_BLOCK, entry);
}

extern "C" int nudf_meshraster_bounds(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_bounds";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_views <= 0 || a.n_faces <= 0) return 0;
  MR_NEED_IMAGE;
  MESH_LAUNCH(mr_bounds_kernel, a.n_views * a.n_faces, MR_BLOCK, MR_BLOCK, entry);
}

extern "C" int nudf_meshraster_draw_small(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_draw_small";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_entries <= 0) return 0;
  MR_NEED_IMAGE;
  MESH_LAUNCH(mr_draw_small_kernel, a.n_entries, MR_BLOCK, MR_BLOCK, entry);
}

extern "C" int nudf_meshraster_draw_large(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_draw_large";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_entries <= 0) return 0;
  MR_NEED_IMAGE;
  MESH_LAUNCH(mr_draw_large_kernel, a.n_entries, MR_BLOCK, MR_BLOCK / MR_WAVE, entry);
}

extern "C" int nudf_meshraster_resolve(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_resolve";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_views <= 0) return 0;
  MR_NEED_IMAGE;
  MESH_LAUNCH(mr_resolve_kernel, (int64_t)a.n_views * a.H * a.W, MR_BLOCK, MR_BLOCK, entry);
}

extern "C" int nudf_meshraster_visible(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_visible";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_views <= 0 || a.n_verts <= 0) return 0;
  MR_NEED_IMAGE;
  MESH_LAUNCH(mr_visible_kernel, a.n_views * a.n_verts, MR_BLOCK, MR_BLOCK, entry);
}

extern "C" int nudf_meshraster_colour(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshraster_colour";
  if (!sizes_ok(a)) return refuse(entry, MR_BAD_SIZES);
  if (a.n_verts <= 0) return 0;
  if (a.n_views > 0) { MR_NEED_IMAGE; }
  MESH_LAUNCH(mr_colour_kernel, a.n_verts, MR_BLOCK, MR_BLOCK, entry);
}
