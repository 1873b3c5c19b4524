// The per-face and per-pixel functions of the rasteriser (csrc/meshraster.hip), shared by draw_small, draw_large and
// resolve so that the three evaluate the same float64 expressions in the same order (include/nudf.h NudfMeshRaster,
// tests/meshraster_ref.py), and the per-point functions -- the depth test of `visible`, the bilinear sample and the view
// weight of `colour` -- that the texture bake (csrc/meshtexture.hip) shares with them, so that a texel at a vertex gets the
// bits the vertex gets.  The including translation unit switches contraction off (f64_exact.h).
#pragma once
#include "f64_exact.h"
#include "nudf_common.h"
#include "../../include/nudf.h"

#define MR_EMPTY 0xffffffffffffffffULL

// q = P p of view `view`: (q.x / q.z, q.y / q.z, q.z)
__device__ __forceinline__ void mr_project(const double* P, const double* p, double* out) {
  const double x = p[0], y = p[1], z = p[2];
  const double qx = add(add(add(mul(P[0], x), mul(P[1], y)), mul(P[2], z)), P[3]);
  const double qy = add(add(add(mul(P[4], x), mul(P[5], y)), mul(P[6], z)), P[7]);
  const double qz = add(add(add(mul(P[8], x), mul(P[9], y)), mul(P[10], z)), P[11]);
  out[0] = __ddiv_rn(qx, qz);
  out[1] = __ddiv_rn(qy, qz);
  out[2] = qz;
}

__device__ __forceinline__ bool mr_valid(const double* s) {
  return is_finite(s[0]) && is_finite(s[1]) && is_finite(s[2]) && s[2] > 0.0;
}

// a face in one view: its three screen vertices and its pixel box, clamped to the image
struct MrFace {
  double x0, y0, z0, x1, y1, z1, x2, y2, z2;
  int32_t xmin, ymin, bw, bh;          // bw * bh = npix
};

// false (and bw = bh = 0) for a face that draws nothing in the view: see `bounds` in include/nudf.h
__device__ __forceinline__ bool mr_face(const NudfMeshRaster& a, int64_t view, int64_t f, MrFace* t) {
  t->bw = t->bh = 0;
  const int64_t* tri = a.faces + 3 * f;
  const int64_t v0 = tri[0], v1 = tri[1], v2 = tri[2];
  if (v0 < 0 || v1 < 0 || v2 < 0 || v0 >= a.n_verts || v1 >= a.n_verts || v2 >= a.n_verts) return false;
  if (v0 == v1 || v1 == v2 || v0 == v2) return false;
  const double* s = a.scr + 3 * view * a.n_verts;
  const double *s0 = s + 3 * v0, *s1 = s + 3 * v1, *s2 = s + 3 * v2;
  if (!mr_valid(s0) || !mr_valid(s1) || !mr_valid(s2)) return false;
  t->x0 = s0[0], t->y0 = s0[1], t->z0 = s0[2];
  t->x1 = s1[0], t->y1 = s1[1], t->z1 = s1[2];
  t->x2 = s2[0], t->y2 = s2[1], t->z2 = s2[2];
  const double area = sub(mul(sub(t->x1, t->x0), sub(t->y2, t->y0)),
                             mul(sub(t->x2, t->x0), sub(t->y1, t->y0)));
  if (!is_finite(area) || area == 0.0) return false;
  // the clamps are taken in float64: the screen coordinates are finite but need not fit an integer
  const double xlo = fmax(ceil(fmin(fmin(t->x0, t->x1), t->x2)), 0.0);
  const double xhi = fmin(floor(fmax(fmax(t->x0, t->x1), t->x2)), (double)(a.W - 1));
  const double ylo = fmax(ceil(fmin(fmin(t->y0, t->y1), t->y2)), 0.0);
  const double yhi = fmin(floor(fmax(fmax(t->y0, t->y1), t->y2)), (double)(a.H - 1));
  if (xlo > xhi || ylo > yhi) return false;
  t->xmin = (int32_t)xlo, t->ymin = (int32_t)ylo;
  t->bw = (int32_t)xhi - t->xmin + 1, t->bh = (int32_t)yhi - t->ymin + 1;
  return true;
}

// the per-pixel function: whether the face covers (px, py) and, where it does, the barycentrics and the depth
__device__ __forceinline__ bool mr_pixel(const MrFace& t, int32_t px, int32_t py, double* b, double* z) {
  const double x = (double)px, y = (double)py;
  const double ax = sub(t.x0, x), ay = sub(t.y0, y);
  const double bx = sub(t.x1, x), by = sub(t.y1, y);
  const double cx = sub(t.x2, x), cy = sub(t.y2, y);
  const double w0 = sub(mul(bx, cy), mul(cx, by));
  const double w1 = sub(mul(cx, ay), mul(ax, cy));
  const double w2 = sub(mul(ax, by), mul(bx, ay));
  if (!((w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0))) return false;
  const double s = add(add(w0, w1), w2);
  if (!is_finite(s) || s == 0.0) return false;
  b[0] = __ddiv_rn(w0, s);
  b[1] = __ddiv_rn(w1, s);
  b[2] = __ddiv_rn(w2, s);
  *z = __ddiv_rn(1.0, add(add(__ddiv_rn(b[0], t.z0), __ddiv_rn(b[1], t.z1)), __ddiv_rn(b[2], t.z2)));
  return true;
}

// draws pixel i (row-major in the box) of face f
__device__ __forceinline__ void mr_draw(const NudfMeshRaster& a, const MrFace& t, int64_t view, int64_t f, int32_t i) {
  const int32_t px = t.xmin + i % t.bw, py = t.ymin + i / t.bw;
  double b[3], z;
  if (!mr_pixel(t, px, py, b, &z)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)z) << 32) | (unsigned long long)f;
  unsigned long long* cell = (unsigned long long*)a.zbuf + (view * a.H + py) * (int64_t)a.W + px;
  // the cell only ever falls: a key that does not beat what a plain load sees cannot beat the cell either
  if (key < __atomic_load_n(cell, __ATOMIC_RELAXED)) atomicMin(cell, key);
}

// ---- a point in a view: what `visible` and `colour` evaluate, and `bake` (csrc/meshtexture.hip) per texel ---------------
// the depth test of `visible` on the projection s of a point: see include/nudf.h
__device__ __forceinline__ bool mr_seen(const NudfMeshRaster& a, int64_t view, const double* s) {
  if (!(mr_valid(s) && fabs(s[0]) < 0x1p52 && fabs(s[1]) < 0x1p52)) return false;
  const double px = rint(s[0]), py = rint(s[1]);     // rint: half to even, as np.round
  if (!(px >= 0.0 && px <= (double)(a.W - 1) && py >= 0.0 && py <= (double)(a.H - 1))) return false;
  const int32_t ix = (int32_t)px, iy = (int32_t)py;
  const int32_t xa = ix > 0 ? ix - 1 : 0, xb = ix < a.W - 1 ? ix + 1 : a.W - 1;
  const int32_t ya = iy > 0 ? iy - 1 : 0, yb = iy < a.H - 1 ? iy + 1 : a.H - 1;
  const float* d = a.depth + view * a.H * (int64_t)a.W;
  float m = d[(int64_t)ya * a.W + xa];
  for (int32_t y = ya; y <= yb; ++y)
    for (int32_t x = xa; x <= xb; ++x) m = fmaxf(m, d[(int64_t)y * a.W + x]);
  return (float)s[2] <= m + a.min_gap;
}

// the four taps of a bilinear sample at (u, w) in a [H, W] image that starts at element `base`: clamped to the image
// whatever u and w are, NaN included
struct MrTaps {
  int64_t p00, p10, p01, p11;
  double w00, w10, w01, w11;
};

__device__ __forceinline__ void mr_taps(double u, double w, int32_t H, int32_t W, int64_t base, MrTaps* t) {
  const double fx0 = floor(u), fy0 = floor(w);
  const double fx = sub(u, fx0), fy = sub(w, fy0);
  const double wmax = (double)(W - 1), hmax = (double)(H - 1);
  const int64_t xa = (int64_t)fmin(fmax(fx0, 0.0), wmax), xb = (int64_t)fmin(fmax(add(fx0, 1.0), 0.0), wmax);
  const int64_t ya = (int64_t)fmin(fmax(fy0, 0.0), hmax), yb = (int64_t)fmin(fmax(add(fy0, 1.0), 0.0), hmax);
  t->p00 = base + ya * W + xa, t->p10 = base + ya * W + xb;
  t->p01 = base + yb * W + xa, t->p11 = base + yb * W + xb;
  const double gx = sub(1.0, fx), gy = sub(1.0, fy);
  t->w00 = mul(gx, gy), t->w10 = mul(fx, gy), t->w01 = mul(gx, fy), t->w11 = mul(fx, fy);
}

__device__ __forceinline__ double mr_mix(const MrTaps& t, double c00, double c10, double c01, double c11) {
  return add(add(mul(t.w00, c00), mul(t.w10, c10)), add(mul(t.w01, c01), mul(t.w11, c11)));
}

// channel c of pixel `pixel` of the source images, in [0, 1] for uint8
__device__ __forceinline__ double mr_tap(const NudfMeshRaster& a, int64_t pixel, int c) {
  if (a.image_f32) return (double)((const float*)a.images)[3 * pixel + c];
  return __ddiv_rn((double)((const uint8_t*)a.images)[3 * pixel + c], 255.0);
}

// pow(|n . d|, power), d the unit direction from p to the camera centre of the view
__device__ __forceinline__ double mr_view_weight(const NudfMeshRaster& a, int64_t view, const double* p, const double* nv) {
  const double* cam = a.cam_pos + 3 * view;
  const double dx = sub(cam[0], p[0]), dy = sub(cam[1], p[1]), dz = sub(cam[2], p[2]);
  const double len = __dsqrt_rn(add(add(mul(dx, dx), mul(dy, dy)), mul(dz, dz)));
  const double dot = add(add(mul(nv[0], __ddiv_rn(dx, len)), mul(nv[1], __ddiv_rn(dy, len))),
                            mul(nv[2], __ddiv_rn(dz, len)));
  return pow(fabs(dot), a.power);
}

// one view's term of the weighted mean at the point p whose projection is s: S += g, C += g c
__device__ __forceinline__ void mr_accumulate(const NudfMeshRaster& a, int64_t view, const double* p, const double* s,
                                              const double* nv, double* sw, double* sc) {
  MrTaps t;
  mr_taps(s[0], s[1], a.H, a.W, view * a.H * (int64_t)a.W, &t);
  const double g = nv ? mr_view_weight(a, view, p, nv) : 1.0;
  for (int c = 0; c < 3; ++c) {
    const double col = mr_mix(t, mr_tap(a, t.p00, c), mr_tap(a, t.p10, c), mr_tap(a, t.p01, c), mr_tap(a, t.p11, c));
    sc[c] = add(sc[c], mul(g, col));
  }
  *sw = add(*sw, g);
}
