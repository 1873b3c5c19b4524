// Texture atlases (include/nudf.h nudf_meshtexture_*, neuraludf_amd/meshrender.py texture_atlas, bake_texture,
// shade_textured): one chart per face, two charts to a power-of-two cell, the cells in Morton order.
//   bake   -- one thread per Morton index of the atlas: the owner face from the class offsets (kernel arguments: the
//             comparison is uniform across almost every wavefront), the texel's point on the face, then over the views in
//             ascending order the depth test of `visible` and the weighted bilinear sample of `colour`, through the same
//             functions (meshraster_pixel.h), so that a texel at a chart corner gets the bits color_vertices gives the
//             vertex.  Neighbouring threads are neighbours in the chart, hence on the surface and in every source image:
//             the kernel is a gather, as `colour` is, and the Morton order is what keeps its taps in the same cache lines;
//   shade  -- one thread per pixel of a raster: the bilinear sample of the texture at the pixel's UV.
// float64 without contraction, no atomics; tests/meshtexture_ref.py restates both operation by operation.
#pragma clang fp contract(off)

#include "meshraster_pixel.h"
#include "mesh_launch.h"

// 256 threads: a 16 x 16 Morton tile of texels, so that a block's depth and image taps fall into a patch of every view; a
// larger block would only straddle more charts.  The bake compiles to 132 VGPRs (3 waves per SIMD): the point, the
// normal, the sums and the taps of one view in float64.  Capping it at 128 for a fourth wave spills 20 bytes per lane;
// which of the two is faster has not been measured.
#define TX_BLOCK 256
#define TX_MAX_CLASSES 10
#define TX_K_MIN 3
#define TX_K_MAX 12

// the even bits of m, packed: the x of a Morton index (its y is tx_even(m >> 1))
__device__ __forceinline__ int32_t tx_even(uint64_t m) {
  m &= 0x5555555555555555ULL;
  m = (m | (m >> 1)) & 0x3333333333333333ULL;
  m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0fULL;
  m = (m | (m >> 4)) & 0x00ff00ff00ff00ffULL;
  m = (m | (m >> 8)) & 0x0000ffff0000ffffULL;
  m = (m | (m >> 16)) & 0x00000000ffffffffULL;
  return (int32_t)m;
}

// the barycentrics of (x, y) in the triangle uv[0..2]: the edge functions of the rasteriser's per-pixel function
__device__ __forceinline__ void tx_bary(const double* uv, double x, double y, double* b) {
  const double ax = sub(uv[0], x), ay = sub(uv[1], y);
  const double bx = sub(uv[2], x), by = sub(uv[3], y);
  const double cx = sub(uv[4], x), cy = sub(uv[5], y);
  const double w0 = sub(mul(bx, cy), mul(cx, by));
  const double w1 = sub(mul(cx, ay), mul(ax, cy));
  const double w2 = sub(mul(ax, by), mul(bx, ay));
  const double s = add(add(w0, w1), w2);
  b[0] = __ddiv_rn(w0, s);
  b[1] = __ddiv_rn(w1, s);
  b[2] = __ddiv_rn(w2, s);
}

__device__ __forceinline__ double tx_mix(const double* b, double x0, double x1, double x2) {
  return add(add(mul(b[0], x0), mul(b[1], x1)), mul(b[2], x2));
}

__device__ __forceinline__ double tx_length(const double* n) {
  return __dsqrt_rn(add(add(mul(n[0], n[0]), mul(n[1], n[1])), mul(n[2], n[2])));
}

// the face that owns Morton index m, -1 when none does
__device__ __forceinline__ int64_t tx_owner(const NudfMeshRaster& a, int64_t m) {
  if (m >= a.tx_class_off[a.tx_n_classes]) return -1;
  int c = 0;
  for (int i = 1; i < TX_MAX_CLASSES; ++i)
    if (i < a.tx_n_classes && a.tx_class_off[i] <= m) c = i;
  const int k = a.tx_class_k[c];
  const int64_t r = m - a.tx_class_off[c];
  const int64_t cell = a.tx_class_cell[c] + (r >> (2 * k));
  if (cell >= a.tx_n_cells) return -1;
  const uint64_t local = (uint64_t)r & ((1ULL << (2 * k)) - 1);
  const int32_t li = tx_even(local), lj = tx_even(local >> 1);
  const int64_t f = a.tx_cell_face[2 * cell + (li + lj <= (1 << k) - 1 ? 0 : 1)];
  return f >= 0 && f < a.n_faces ? f : -1;
}

__global__ __launch_bounds__(TX_BLOCK) void tx_bake_kernel(NudfMeshRaster a) {
  const int64_t m = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
  if (m >= (int64_t)a.tx_W * a.tx_H) return;
  const int32_t i = tx_even((uint64_t)m), j = tx_even((uint64_t)m >> 1);
  if (i >= a.tx_W || j >= a.tx_H) return;              // (never: the atlas is the Morton range [0, W H))
  const int64_t texel = (int64_t)j * a.tx_W + i;
  float out[3] = {a.fill[0], a.fill[1], a.fill[2]};
  int32_t seen = -1;
  const int64_t f = tx_owner(a, m);
  if (f >= 0) {
    seen = 0;
    const int64_t* tri = a.faces + 3 * f;
    const int64_t v0 = tri[0], v1 = tri[1], v2 = tri[2];
    if (v0 >= 0 && v1 >= 0 && v2 >= 0 && v0 < a.n_verts && v1 < a.n_verts && v2 < a.n_verts) {
      double b[3], p[3], nv[3];
      tx_bary(a.tx_uv + 6 * f, (double)i, (double)j, b);
      const double *p0 = a.pos + 3 * v0, *p1 = a.pos + 3 * v1, *p2 = a.pos + 3 * v2;
      for (int c = 0; c < 3; ++c) p[c] = tx_mix(b, p0[c], p1[c], p2[c]);
      if (a.normals) {
        const double *n0 = a.normals + 3 * v0, *n1 = a.normals + 3 * v1, *n2 = a.normals + 3 * v2;
        double mixed[3];
        for (int c = 0; c < 3; ++c) mixed[c] = tx_mix(b, n0[c], n1[c], n2[c]);
        const double len = tx_length(mixed);
        const double t = len > 0.0 ? __ddiv_rn(tx_mix(b, tx_length(n0), tx_length(n1), tx_length(n2)), len) : 0.0;
        for (int c = 0; c < 3; ++c) nv[c] = mul(mixed[c], t);
      }
      double sw = 0.0, sc[3] = {0.0, 0.0, 0.0};
      int32_t n = 0;
      for (int64_t view = 0; view < a.n_views; ++view) {
        double s[3];
        mr_project(a.proj + 12 * view, p, s);
        if (!mr_seen(a, view, s)) continue;
        mr_accumulate(a, view, p, s, a.normals ? nv : nullptr, &sw, sc);
        ++n;
      }
      if (sw > 0.0 && sw < HUGE_VAL) {
        seen = n;
        for (int c = 0; c < 3; ++c) out[c] = (float)__ddiv_rn(sc[c], sw);
      } else if (a.tx_fallback) {
        const float *c0 = a.tx_fallback + 3 * v0, *c1 = a.tx_fallback + 3 * v1, *c2 = a.tx_fallback + 3 * v2;
        for (int c = 0; c < 3; ++c) out[c] = (float)tx_mix(b, (double)c0[c], (double)c1[c], (double)c2[c]);
      }
    }
  }
  for (int c = 0; c < 3; ++c) a.tx_colors[3 * texel + c] = out[c];
  a.tx_n_seen[texel] = seen;
}

__global__ __launch_bounds__(TX_BLOCK) void tx_shade_kernel(NudfMeshRaster a) {
  const int64_t px = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
  if (px >= (int64_t)a.n_views * a.H * a.W) return;
  const int64_t f = a.face[px];
  float out[3] = {a.tx_background[0], a.tx_background[1], a.tx_background[2]};
  if (f >= 0 && f < a.n_faces) {
    const double b[3] = {(double)a.bary[3 * px], (double)a.bary[3 * px + 1], (double)a.bary[3 * px + 2]};
    const double* uv = a.tx_uv + 6 * f;
    MrTaps t;
    mr_taps(tx_mix(b, uv[0], uv[2], uv[4]), tx_mix(b, uv[1], uv[3], uv[5]), a.tx_H, a.tx_W, 0, &t);
    const float* tex = a.tx_colors;
    for (int c = 0; c < 3; ++c)
      out[c] = (float)mr_mix(t, (double)tex[3 * t.p00 + c], (double)tex[3 * t.p10 + c], (double)tex[3 * t.p01 + c],
                             (double)tex[3 * t.p11 + c]);
  }
  for (int c = 0; c < 3; ++c) a.tx_out[3 * px + c] = out[c];
}

// ---- launchers --------------------------------------------------------------------------------------------------------
#define TX_MAX_THREADS (1LL << 38)                   // one-dimensional grids of TX_BLOCK threads: < 2^31 blocks

static const char* sizes_bad(const NudfMeshRaster& a) {
  if (a.n_faces < 0 || a.n_faces >= (1LL << 31) || a.n_verts < 0 || a.n_verts >= (1LL << 31))
    return "n_faces and n_verts must be in [0, 2^31)";
  if (a.n_views < 0 || a.H < 0 || a.W < 0) return "n_views, H and W must be >= 0";
  if ((int64_t)a.H * a.W >= (1LL << 31)) return "H * W must be < 2^31";
  if ((int64_t)a.n_views * a.H * a.W > TX_MAX_THREADS) return "n_views * H * W must be <= 2^38";
  if (a.tx_W < 0 || a.tx_H < 0) return "tx_W and tx_H must be >= 0";
  if ((int64_t)a.tx_W * a.tx_H >= (1LL << 31)) return "tx_W * tx_H must be < 2^31";
  if (a.tx_n_cells < 0) return "tx_n_cells must be >= 0";
  return nullptr;
}

static const char* classes_bad(const NudfMeshRaster& a) {
  if (a.tx_n_classes < 0 || a.tx_n_classes > TX_MAX_CLASSES) return "tx_n_classes must be in [0, 10]";
  if (a.tx_class_off[0] != 0 || a.tx_class_cell[0] != 0) return "tx_class_off and tx_class_cell must start at 0";
  for (int c = 0; c < a.tx_n_classes; ++c) {
    if (a.tx_class_k[c] < TX_K_MIN || a.tx_class_k[c] > TX_K_MAX) return "every tx_class_k must be in [3, 12]";
    if (a.tx_class_off[c + 1] < a.tx_class_off[c] || a.tx_class_cell[c + 1] < a.tx_class_cell[c])
      return "tx_class_off and tx_class_cell must ascend";
  }
  return nullptr;
}

extern "C" int nudf_meshtexture_bake(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshtexture_bake";
  if (const char* why = sizes_bad(a)) return refuse(entry, why);
  if (const char* why = classes_bad(a)) return refuse(entry, why);
  const int64_t n = (int64_t)a.tx_W * a.tx_H;
  if (n <= 0) return 0;
  if (!a.tx_colors || !a.tx_n_seen) return refuse(entry, "tx_colors and tx_n_seen must not be NULL");
  if (a.tx_n_classes > 0 && a.tx_n_cells > 0) {          // otherwise no texel has an owner: nothing else is read
    if (!a.tx_uv || !a.tx_cell_face || !a.faces || !a.pos)
      return refuse(entry, "tx_uv, tx_cell_face, faces and pos must not be NULL");
    if (a.n_views > 0 && a.n_faces > 0) {
      if (a.H < 1 || a.W < 1) return refuse(entry, "H and W must be >= 1");
      if (!a.proj || !a.depth || !a.images) return refuse(entry, "proj, depth and images must not be NULL");
      if (a.normals && !a.cam_pos) return refuse(entry, "cam_pos must not be NULL with normals");
      if (a.normals && !(a.power - a.power == 0.0)) return refuse(entry, "power must be finite");
    }
  }
  MESH_LAUNCH(tx_bake_kernel, n, TX_BLOCK, TX_BLOCK, entry);
}

extern "C" int nudf_meshtexture_shade(const NudfMeshRaster* args, void* stream) {
  const NudfMeshRaster& a = *args;
  const char* const entry = "nudf_meshtexture_shade";
  if (const char* why = sizes_bad(a)) return refuse(entry, why);
  const int64_t n = (int64_t)a.n_views * a.H * a.W;
  if (n <= 0) return 0;
  if (a.tx_W < 1 || a.tx_H < 1) return refuse(entry, "tx_W and tx_H must be >= 1");
  if (!a.face || !a.bary || !a.tx_out || !a.tx_colors) return refuse(entry, "face, bary, tx_colors and tx_out must not be NULL");
  if (a.n_faces > 0 && !a.tx_uv) return refuse(entry, "tx_uv must not be NULL");
  MESH_LAUNCH(tx_shade_kernel, n, TX_BLOCK, TX_BLOCK, entry);
}
