// The per-cell and per-edge arithmetic of the MeshUDF mesher, shared by the dense kernels (meshudf.hip) and the sparse
// ones (meshudf_sparse.hip) so that both decide every cell and place every vertex with the same instructions: the active
// test, the largest-corner reference, the float64 dot with explicit roundings, the case index, the triangle count, the
// sign-change test of an edge and the vertex interpolation.  Needs mc_tables.inc included before it.
#pragma once

// case index of a cell (bit c set: corner c is `-`) and its triangle count `nt`; 0 / 0 for an inactive cell.  u: the 8
// corner values (corner bits: 4 = x, 2 = y, 1 = z); grad(c): pointer to the 3 gradient components of corner c, called for
// the corners of active cells only.
template <class Grad>
__device__ __forceinline__ uint32_t meshudf_cell_case(const float (&u)[8], float mean_thr, float max_thr, Grad grad,
                                                      uint32_t& nt) {
  float sum = u[0];
  int r = 0;                                    // reference corner: largest U, lowest index on ties
#pragma unroll
  for (int c = 1; c < 8; ++c) {
    sum = __fadd_rn(sum, u[c]);
    if (u[c] > u[r]) r = c;
  }
  uint32_t cs = 0;
  nt = 0;
  if (__fmul_rn(sum, 0.125f) < mean_thr && u[r] <= max_thr) {
    const float* gr = grad(r);
    const double rx = gr[0], ry = gr[1], rz = gr[2];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c == r) continue;
      const float* g = grad(c);
      const double d = __dadd_rn(__dadd_rn(__dmul_rn(rx, (double)g[0]), __dmul_rn(ry, (double)g[1])),
                                 __dmul_rn(rz, (double)g[2]));
      if (!(d >= 0.0)) cs |= 1u << c;
    }
    nt = nudf_mc_ntri[cs];
  }
  return cs;
}

// does edge e of a cell with case index cs join a `+` and a `-` corner
__device__ __forceinline__ bool meshudf_edge_crossed(uint32_t cs, int e) {
  const int lo = nudf_mc_edge[e][0] * 4 + nudf_mc_edge[e][1] * 2 + nudf_mc_edge[e][2];
  const int hi = lo | (4 >> nudf_mc_edge[e][3]);
  return (((cs >> lo) ^ (cs >> hi)) & 1) != 0;
}

// weight of the vertex on an edge from its lower end a: U_a / (U_a + U_b), 0.5 where both are 0
__device__ __forceinline__ float meshudf_vertex_weight(float ua, float ub) {
  const float s = __fadd_rn(ua, ub);
  return s == 0.0f ? 0.5f : __fdiv_rn(ua, s);
}

// coordinate of that vertex along the edge's axis between the grid coordinates xa (lower end) and xb
__device__ __forceinline__ float meshudf_vertex_coord(float xa, float xb, float w) {
  return __fadd_rn(xa, __fmul_rn(w, __fsub_rn(xb, xa)));
}
