// The hashed uniform grid of include/nudf.h NudfPointCloud, in one place: pointcloud.hip builds it (keys, cells) and
// searches it for points, meshdist.hip bins faces into it and searches it for the closest face, meshray.hip walks rays
// through it.  A table built by one file is searched by the others, so a cell coordinate, a key and a probe sequence
// must be the same numbers everywhere: they are defined here and nowhere else.
// The including translation unit switches contraction off (f64_exact.h).
#pragma once
#include "f64_exact.h"
#include "../../include/nudf.h"

#define PC_AXIS_BITS 21
#define PC_AXIS_MAX ((1 << PC_AXIS_BITS) - 1)
#define PC_EMPTY (-1LL)
// a cell coordinate is computed with a relative error of a few ulps of its value (< 2^22): at most 2^-29 of a cell.  The
// ring search, the ray walk and the thinning's 27-cell window allow 2^-20 of a cell for it.
#define PC_CELL_MARGIN 0x1p-20

// cell coordinate of x along one axis, unclamped (a query may lie outside the points' box); |value| <= 2^30
__device__ __forceinline__ int64_t cell_coord(double x, double origin, double cell) {
  double u = floor(__ddiv_rn(sub(x, origin), cell));
  u = u < -0x1p30 ? -0x1p30 : (u > 0x1p30 ? 0x1p30 : u);   // far outside the grid: the ring bound still holds
  return (int64_t)u;
}

__device__ __forceinline__ int64_t pack_key(int64_t x, int64_t y, int64_t z) {
  return (x << (2 * PC_AXIS_BITS)) | (y << PC_AXIS_BITS) | z;
}

__device__ __forceinline__ int64_t clamp_axis(int64_t c) { return c < 0 ? 0 : (c > PC_AXIS_MAX ? PC_AXIS_MAX : c); }

__device__ __forceinline__ uint64_t hash_mix(uint64_t k) {    // the murmur3 64-bit finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

// the probe sequence of `key` in a table of mask + 1 slots (a power of two): insertion and lookup walk the same one
__device__ __forceinline__ uint64_t probe_first(int64_t key, uint64_t mask) { return hash_mix((uint64_t)key) & mask; }
__device__ __forceinline__ uint64_t probe_next(uint64_t h, uint64_t mask) { return (h + 1) & mask; }

// row of the sorted cell table holding `key`, or -1 (the table is at most half full: a probe always meets an empty slot)
__device__ int64_t cell_row(const NudfPointCloud& a, int64_t key) {
  const uint64_t mask = (uint64_t)a.hash_cap - 1;
  uint64_t h = probe_first(key, mask);
  for (int64_t probe = 0; probe < a.hash_cap; ++probe) {
    const int64_t k = a.hash_key[h];
    if (k == key) return a.hash_row[h];
    if (k == PC_EMPTY) return -1;
    h = probe_next(h, mask);
  }
  return -1;
}

// ---- the ring walk -------------------------------------------------------------------------------------------------------
// Rings k = k0, k0 + 1, ... of cells at Chebyshev distance k from the query's cell; k0 > 0 for a query outside the grid.
// visit(x, y, z) is called once on every cell of the grid that a ring adds; best() is the smallest distance met so far.
// Once the rings up to k are done, everything not met lies more than (k - margin) cells from the query: the walk stops
// when best() is below that (no tie can come later), when that exceeds `bound`, or when the rings cover the grid.  A query
// farther than the bound from the box of the data (box_lo, box_hi, box_bound2) visits nothing.
template <class Visit, class Best>
__device__ __forceinline__ void ring_walk(const NudfPointCloud& a, double qx, double qy, double qz, Visit&& visit,
                                          Best&& best) {
  const double bx = fmax(fmax(sub(a.box_lo[0], qx), sub(qx, a.box_hi[0])), 0.0);
  const double by = fmax(fmax(sub(a.box_lo[1], qy), sub(qy, a.box_hi[1])), 0.0);
  const double bz = fmax(fmax(sub(a.box_lo[2], qz), sub(qz, a.box_hi[2])), 0.0);
  if (dot3(bx, by, bz) > a.box_bound2) return;
  const int64_t c[3] = {cell_coord(qx, a.origin[0], a.cell), cell_coord(qy, a.origin[1], a.cell),
                        cell_coord(qz, a.origin[2], a.cell)};
  int64_t k = 0;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const int64_t off = c[x] < 0 ? -c[x] : (c[x] >= a.grid[x] ? c[x] - (a.grid[x] - 1) : 0);
    k = off > k ? off : k;
  }
  for (;; ++k) {
    const int64_t x0 = c[0] - k < 0 ? 0 : c[0] - k, x1 = c[0] + k >= a.grid[0] ? a.grid[0] - 1 : c[0] + k;
    const int64_t y0 = c[1] - k < 0 ? 0 : c[1] - k, y1 = c[1] + k >= a.grid[1] ? a.grid[1] - 1 : c[1] + k;
    const int64_t z0 = c[2] - k < 0 ? 0 : c[2] - k, z1 = c[2] + k >= a.grid[2] ? a.grid[2] - 1 : c[2] + k;
    for (int64_t x = x0; x <= x1; ++x) {
      for (int64_t y = y0; y <= y1; ++y) {
        if (x == c[0] - k || x == c[0] + k || y == c[1] - k || y == c[1] + k) {
          for (int64_t z = z0; z <= z1; ++z) visit(x, y, z);
        } else {                                   // k >= 1: only the ring's two z faces are new in this column
          if (c[2] - k >= 0) visit(x, y, c[2] - k);
          if (c[2] + k < a.grid[2]) visit(x, y, c[2] + k);
        }
      }
    }
    const double reach = mul(sub((double)k, PC_CELL_MARGIN), a.cell);
    if (best() < reach || reach > a.bound) break;
    if (c[0] - k <= 0 && c[1] - k <= 0 && c[2] - k <= 0 && c[0] + k >= a.grid[0] - 1 && c[1] + k >= a.grid[1] - 1 &&
        c[2] + k >= a.grid[2] - 1)
      break;                                             // every cell has been seen
  }
}

// ---- what a launcher checks of the grid on the host ------------------------------------------------------------------------
static inline bool grid_ok(const NudfPointCloud& a) {      // every axis in [1, 2^21]
  for (int x = 0; x < 3; ++x)
    if (a.grid[x] < 1 || a.grid[x] > PC_AXIS_MAX + 1) return false;
  return true;
}

static inline bool origin_ok(const NudfPointCloud& a) {    // finite
  for (int x = 0; x < 3; ++x)
    if (!(a.origin[x] - a.origin[x] == 0.0)) return false;
  return true;
}
