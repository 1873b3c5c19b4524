// The per-cell and per-edge arithmetic of the level-set mesher, shared by its dense and sparse kernels (isosurface.hip)
// so that both decide every cell and place every vertex with the same instructions: the sign rule, the non-finite test,
// the case index, the triangle count and the vertex interpolation.  The sign-change test of an edge and the coordinate
// form are the MeshUDF mesher's (meshudf_cell.h).  Needs mc_tables.inc included before it.
#pragma once
#include "meshudf_cell.h"

// NaN, +inf or -inf
__device__ __forceinline__ bool iso_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// case index of a cell (bit c set: corner c is `-`, i.e. f[c] < level) and its triangle count `nt`; 0 / 0 for a cell with
// a non-finite corner.  f: the 8 corner values (corner bits: 4 = x, 2 = y, 1 = z).
__device__ __forceinline__ uint32_t iso_cell_case(const float (&f)[8], float level, uint32_t& nt) {
  uint32_t cs = 0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    bad |= iso_nonfinite(f[c]);
    cs |= (f[c] < level ? 1u : 0u) << c;
  }
  if (bad) cs = 0;
  nt = nudf_mc_ntri[cs];
  return cs;
}

// weight of the vertex on an edge from its lower end a: (level - F_a) / (F_b - F_a), clamped to [0, 1]; 0.5 where that
// is NaN
__device__ __forceinline__ float iso_vertex_weight(float fa, float fb, float level) {
  const float t = __fdiv_rn(__fsub_rn(level, fa), __fsub_rn(fb, fa));
  if (t != t) return 0.5f;
  return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
}
