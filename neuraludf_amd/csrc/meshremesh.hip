// Isotropic remeshing (include/nudf.h NudfMeshTopo sp_sd_hf_rm_ fields, neuraludf_amd/meshclean.py remesh_isotropic): the
// two local operations the library lacked, collapsing and flipping an edge, and the tangential relaxation of Botsch and
// Kobbelt's loop (2004); the split is meshsubdiv.hip's, the projection meshdist.hip's.  What the reference's users leave
// the GPU for with pymeshlab, CGAL or trimesh.remesh.
//   collapse_check  -- one thread per edge: is it short, do its ends allow it, does the link condition hold, does no edge
//                      grow beyond the bound and no face turn over;
//   vertex_min      -- one thread per vertex: the smallest rank of a candidate at the vertex, around it, or on its faces;
//   collapse_apply  -- one thread per edge: the candidates that hold the minimum of their neighbourhood are collapsed;
//   flip_check      -- one thread per edge: does the flip bring the valences nearer their targets without a fold;
//   flip_apply      -- one thread per edge: the candidates that hold the minimum at all four corners are flipped;
//   relax           -- one thread per vertex: the one-ring's mean, moved back into the tangent plane.
// Winners are an independent set taken by minimum passes over unique ranks (the argument is in the header): every thread
// writes its own item or rows that no other winner touches, no atomics, identical from run to run.  The float64
// expressions follow the numpy restatement (tests/meshremesh_ref.py) operation by operation: products and sums go through
// mul / add / sub of f64_exact.h under the pragma; square roots and quotients are the correctly rounded __dsqrt_rn and
// __ddiv_rn.  The walks are loops over CSR ranges: no local arrays, no scratch memory.
#pragma clang fp contract(off)

#include "f64_exact.h"
#include "mesh_launch.h"
#include "../../include/nudf.h"

#define RM_BLOCK 256

__device__ __forceinline__ bool vertex_ok(const NudfMeshTopo& a, int64_t v) { return v >= 0 && v < a.n_verts; }

__device__ __forceinline__ bool in_range(const NudfMeshTopo& a, const int64_t* t) {
  return vertex_ok(a, t[0]) && vertex_ok(a, t[1]) && vertex_ok(a, t[2]);
}

__device__ __forceinline__ double dist2(const V3& p, const V3& q) {
  const V3 d = vsub(p, q);
  return dot3(d.x, d.y, d.z);
}

// the position of vertex w, or `moved` when w is one of the two ends that a collapse merges (g0 = g1 = -1: nothing moves)
__device__ __forceinline__ V3 place(const NudfMeshTopo& a, int64_t w, int64_t g0, int64_t g1, V3 moved) {
  const bool merged = w == g0 || w == g1;
  const double* p = a.pos + 3 * w;
  return {merged ? moved.x : p[0], merged ? moved.y : p[1], merged ? moved.z : p[2]};
}

// (p1 - p0) x (p2 - p0) of the corners (t0, t1, t2), rotated so that the smallest index comes first
__device__ __forceinline__ V3 normal_of(const NudfMeshTopo& a, int64_t t0, int64_t t1, int64_t t2, int64_t g0, int64_t g1,
                                        V3 moved) {
  int64_t i0 = t0, i1 = t1, i2 = t2;
  if (t1 < t0 && t1 <= t2) i0 = t1, i1 = t2, i2 = t0;
  else if (t2 < t0 && t2 < t1) i0 = t2, i1 = t0, i2 = t1;
  const V3 p0 = place(a, i0, g0, g1, moved);
  return vcross(vsub(place(a, i1, g0, g1, moved), p0), vsub(place(a, i2, g0, g1, moved), p0));
}

// the vertex opposite half-edge h in its face, or -1
__device__ __forceinline__ int64_t opposite(const NudfMeshTopo& a, int64_t h) {
  if (h < 0 || h >= 3 * a.n_faces) return -1;
  const int64_t w = a.faces[h / 3 * 3 + (h % 3 + 2) % 3];
  return vertex_ok(a, w) ? w : -1;
}

// the CSR range of w in a table of `total` entries: false when it does not lie inside
__device__ __forceinline__ bool csr_range(const int64_t* off, int64_t w, int64_t total, int64_t* b, int64_t* e) {
  *b = off[w];
  *e = off[w + 1];
  return *b >= 0 && *e >= *b && *e <= total;
}

// ---- (a) may the edge be collapsed ---------------------------------------------------------------------------------------
// the common vertices of the two ascending one-rings, -1 when a range is out of the table
__device__ __forceinline__ int64_t common_ring(const NudfMeshTopo& a, int64_t u, int64_t v) {
  int64_t i, ie, j, je;
  if (!csr_range(a.sp_sd_ring_off, u, a.sp_sd_n_ring, &i, &ie) || !csr_range(a.sp_sd_ring_off, v, a.sp_sd_n_ring, &j, &je)) return -1;
  int64_t n = 0;
  while (i < ie && j < je) {
    const int64_t x = a.sp_sd_ring[i], y = a.sp_sd_ring[j];
    if (x == y) ++n, ++i, ++j;
    else if (x < y) ++i;
    else ++j;
  }
  return n;
}

// the border test of removing g towards k: g's other border neighbour turns by less than the bound and is not `apex`
__device__ __forceinline__ bool border_ok(const NudfMeshTopo& a, int64_t g, int64_t k, int64_t apex) {
  int64_t b, e;
  if (!csr_range(a.nbr_off, g, a.sp_sd_n_border, &b, &e) || e - b != 2) return false;
  const int64_t b0 = a.nbr[b], b1 = a.nbr[b + 1];
  const int64_t o = b0 == k ? b1 : (b1 == k ? b0 : -1);
  if (!vertex_ok(a, o) || o == k || o == g || o == apex) return false;
  if (!(a.sp_sd_hf_rm_cos_border < 1.0)) return false;
  const V3 pg = vload(a.pos + 3 * g);
  const V3 in = vsub(pg, vload(a.pos + 3 * o)), out = vsub(vload(a.pos + 3 * k), pg);
  const double bound = mul(mul(a.sp_sd_hf_rm_cos_border, __dsqrt_rn(dot3(in.x, in.y, in.z))), __dsqrt_rn(dot3(out.x, out.y, out.z)));
  return vdot(in, out) > bound;
}

// _CLASS, _REACH, _FOLD, _DUPLICATE or 0 for the ends u, v merged at p, `gone` the one that is removed; (ca, cb) the
// corners opposite an edge with two faces, else -1
__device__ __forceinline__ int collapse_geometry(const NudfMeshTopo& a, int64_t u, int64_t v, int64_t gone, V3 p, int64_t ca,
                                                 int64_t cb) {
  const double high2 = mul(a.sp_sd_hf_rm_high, a.sp_sd_hf_rm_high);
  {
    int64_t b, e;
    if (!csr_range(a.sp_sd_ring_off, gone, a.sp_sd_n_ring, &b, &e)) return NUDF_REMESH_CLASS;
    for (int64_t j = b; j < e; ++j) {                                          // a vertex that stays keeps its faces
      const int64_t x = a.sp_sd_ring[j];
      if (!vertex_ok(a, x) || a.sp_sd_vclass[x] > 1) return NUDF_REMESH_CLASS;
    }
  }
  for (int side = 0; side < 2; ++side) {
    int64_t b, e;
    if (!csr_range(a.sp_sd_ring_off, side ? v : u, a.sp_sd_n_ring, &b, &e)) return NUDF_REMESH_REACH;
    for (int64_t j = b; j < e; ++j) {
      const int64_t x = a.sp_sd_ring[j];
      if (x == u || x == v) continue;
      if (!vertex_ok(a, x) || !(dist2(vload(a.pos + 3 * x), p) <= high2)) return NUDF_REMESH_REACH;
    }
  }
  bool twin_u = false, twin_v = false;
  for (int side = 0; side < 2; ++side) {
    const int64_t w = side ? v : u;
    int64_t b, e;
    if (!csr_range(a.sp_sd_hf_rm_corner_off, w, 3 * a.n_faces, &b, &e)) return NUDF_REMESH_FOLD;
    for (int64_t j = b; j < e; ++j) {
      const int64_t c = a.sp_sd_hf_rm_corner[j];
      if (c < 0 || c >= 3 * a.n_faces) return NUDF_REMESH_FOLD;
      const int64_t* t = a.faces + c / 3 * 3;
      if (!in_range(a, t)) return NUDF_REMESH_FOLD;
      const bool has_u = t[0] == u || t[1] == u || t[2] == u, has_v = t[0] == v || t[1] == v || t[2] == v;
      if (has_u && has_v) continue;                                          // the face goes with the edge
      const V3 before = normal_of(a, t[0], t[1], t[2], -1, -1, p), after = normal_of(a, t[0], t[1], t[2], u, v, p);
      if (!(vdot(before, after) > 0.0)) return NUDF_REMESH_FOLD;
      const int k = c % 3;
      const int64_t x = t[(k + 1) % 3], y = t[(k + 2) % 3];
      const bool twin = ca >= 0 && t[k] == w && ((x == ca && y == cb) || (x == cb && y == ca));
      twin_u = twin_u || (twin && side == 0);
      twin_v = twin_v || (twin && side == 1);
    }
  }
  return twin_u && twin_v ? NUDF_REMESH_DUPLICATE : NUDF_REMESH_CANDIDATE;
}

__device__ __forceinline__ V3 midpoint(const V3& p, const V3& q) {
  return {mul(add(p.x, q.x), 0.5), mul(add(p.y, q.y), 0.5), mul(add(p.z, q.z), 0.5)};
}

// an edge with two faces whose ends are both smooth: the kept end u moves to the midpoint; every other kept end stays
__device__ __forceinline__ bool moves_to_midpoint(const NudfMeshTopo& a, int64_t e) {
  return a.edges[5 * e + 2] == 2 && a.sp_sd_vclass[a.edges[5 * e]] == 0 && a.sp_sd_vclass[a.edges[5 * e + 1]] == 0;
}

__global__ __launch_bounds__(RM_BLOCK) void rm_collapse_check_kernel(NudfMeshTopo a) {
  const int64_t e = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
  if (e >= a.n_edges) return;
  const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1], count = a.edges[5 * e + 2];
  int status = NUDF_REMESH_CANDIDATE;
  int64_t keep = -1, gone = -1;
  const int64_t s = a.edge_start[e];
  if ((count != 1 && count != 2) || u == v || !vertex_ok(a, u) || !vertex_ok(a, v) || s < 0 || s + count > 3 * a.n_faces) {
    status = NUDF_REMESH_COUNT;
  } else {
    const V3 pu = vload(a.pos + 3 * u), pv = vload(a.pos + 3 * v);
    const int cu = a.sp_sd_vclass[u], cv = a.sp_sd_vclass[v];
    const int64_t ca = opposite(a, a.he_id[s]), cb = count == 2 ? opposite(a, a.he_id[s + 1]) : -1;
    if (!(dist2(pu, pv) < mul(a.sp_sd_hf_rm_low, a.sp_sd_hf_rm_low))) {
      status = NUDF_REMESH_LONG;
    } else if (cu > 1 || cv > 1) {
      status = NUDF_REMESH_CLASS;
    } else if (count == 2) {
      if (cu == 1 && cv == 1) {
        status = NUDF_REMESH_BORDER;
      } else if (common_ring(a, u, v) != 2) {
        status = NUDF_REMESH_LINK;
      } else {
        keep = cv == 1 ? v : u;
        gone = cv == 1 ? u : v;
        status = collapse_geometry(a, u, v, gone, cu == 1 ? pu : (cv == 1 ? pv : midpoint(pu, pv)), ca, cb);
      }
    } else {
      const bool first = border_ok(a, v, u, ca), second = border_ok(a, u, v, ca);      // (keep u, remove v), (keep v, remove u)
      if (!first && !second) {
        status = NUDF_REMESH_BORDER;
      } else if (common_ring(a, u, v) != 1) {
        status = NUDF_REMESH_LINK;
      } else {
        status = first ? collapse_geometry(a, u, v, v, pu, -1, -1) : NUDF_REMESH_BORDER;
        keep = u, gone = v;
        if (status != NUDF_REMESH_CANDIDATE && second) {
          const int other = collapse_geometry(a, u, v, u, pv, -1, -1);
          if (other == NUDF_REMESH_CANDIDATE || !first) status = other;
          if (other == NUDF_REMESH_CANDIDATE) keep = v, gone = u;
        }
      }
    }
  }
  const bool candidate = status == NUDF_REMESH_CANDIDATE;
  a.sp_sd_hf_rm_status[e] = (uint8_t)status;
  a.sp_sd_hf_rm_keep[e] = candidate ? keep : -1;
  a.sp_sd_hf_rm_gone[e] = candidate ? gone : -1;
}

// ---- (b) the minimum passes ----------------------------------------------------------------------------------------------
// the rank of edge e when it is a candidate, else "none"
__device__ __forceinline__ int64_t rank_of(const NudfMeshTopo& a, int64_t e) {
  if (e < 0 || e >= a.n_edges || a.sp_sd_hf_rm_status[e] != NUDF_REMESH_CANDIDATE) return a.n_edges;
  const int64_t r = a.sp_sd_hf_rm_rank[e];
  return r >= 0 && r < a.n_edges ? r : a.n_edges;
}

__global__ __launch_bounds__(RM_BLOCK) void rm_vertex_min_kernel(NudfMeshTopo a) {
  const int64_t w = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
  if (w >= a.n_verts) return;
  int64_t best = a.n_edges, b, e;
  if (a.sp_sd_hf_rm_mode == 0) {
    if (csr_range(a.sp_sd_hf_rm_vedge_off, w, a.sp_sd_hf_rm_n_vedge, &b, &e))
      for (int64_t j = b; j < e; ++j) {
        const int64_t r = rank_of(a, a.sp_sd_hf_rm_vedge[j]);
        best = r < best ? r : best;
      }
  } else if (a.sp_sd_hf_rm_mode == 1) {
    best = a.sp_sd_hf_rm_best_in[w];
    if (csr_range(a.sp_sd_ring_off, w, a.sp_sd_n_ring, &b, &e))
      for (int64_t j = b; j < e; ++j) {
        const int64_t x = a.sp_sd_ring[j];
        if (!vertex_ok(a, x)) continue;
        const int64_t r = a.sp_sd_hf_rm_best_in[x];
        best = r < best ? r : best;
      }
  } else {
    if (csr_range(a.sp_sd_hf_rm_corner_off, w, 3 * a.n_faces, &b, &e))
      for (int64_t j = b; j < e; ++j) {
        const int64_t c = a.sp_sd_hf_rm_corner[j];
        if (c < 0 || c >= 3 * a.n_faces) continue;
        for (int k = 0; k < 3; ++k) {
          const int64_t r = rank_of(a, a.he_edge[c / 3 * 3 + k]);
          best = r < best ? r : best;
        }
      }
  }
  a.sp_sd_hf_rm_best_out[w] = best;
}

// ---- (c) the winning collapses -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_BLOCK) void rm_collapse_apply_kernel(NudfMeshTopo a) {
  const int64_t e = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
  if (e >= a.n_edges) return;
  uint8_t win = 0;
  const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1], r = rank_of(a, e);
  if (r < a.n_edges && vertex_ok(a, u) && vertex_ok(a, v) && u != v) {
    const int64_t bu = a.sp_sd_hf_rm_best_in[u], bv = a.sp_sd_hf_rm_best_in[v];
    const int64_t keep = a.sp_sd_hf_rm_keep[e], gone = a.sp_sd_hf_rm_gone[e];
    if (r == (bu < bv ? bu : bv) && ((keep == u && gone == v) || (keep == v && gone == u))) {
      win = 1;
      a.sp_sd_hf_rm_remap[gone] = keep;
      const V3 pk = vload(a.pos + 3 * keep);
      const V3 p = moves_to_midpoint(a, e) ? midpoint(vload(a.pos + 3 * u), vload(a.pos + 3 * v)) : pk;
      double* o = a.sp_sd_hf_rm_pos_out + 3 * keep;
      o[0] = p.x, o[1] = p.y, o[2] = p.z;
    }
  }
  a.sp_sd_hf_rm_win[e] = win;
}

// ---- (d) may the edge be flipped ------------------------------------------------------------------------------------------
// position of `key` in the ascending edge_key, or -1
__device__ __forceinline__ int64_t find_edge(const NudfMeshTopo& a, int64_t key) {
  int64_t lo = 0, hi = a.n_edges;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a.edge_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.n_edges && a.edge_key[lo] == key ? lo : -1;
}

// (valence + shift - target)^2 of vertex w; a one-ring outside the table counts as empty
__device__ __forceinline__ int64_t deviation2(const NudfMeshTopo& a, int64_t w, int64_t shift) {
  int64_t b, e;
  const int64_t n = csr_range(a.sp_sd_ring_off, w, a.sp_sd_n_ring, &b, &e) ? e - b : 0;
  const int64_t d = n + shift - (a.sp_sd_vclass[w] == 1 ? 4 : 6);
  return d * d;
}

// the two half-edges and faces of an edge with two faces: false when a table entry is out of range or a face repeats
struct Wings {
  int64_t h0, h1, ca, cb;
};
__device__ __forceinline__ bool wings_of(const NudfMeshTopo& a, int64_t e, Wings* w) {
  const int64_t s = a.edge_start[e];
  if (s < 0 || s + 2 > 3 * a.n_faces) return false;
  w->h0 = a.he_id[s];
  w->h1 = a.he_id[s + 1];
  w->ca = opposite(a, w->h0);
  w->cb = opposite(a, w->h1);
  return w->ca >= 0 && w->cb >= 0 && w->h0 / 3 != w->h1 / 3 && in_range(a, a.faces + w->h0 / 3 * 3) && in_range(a, a.faces + w->h1 / 3 * 3);
}

__global__ __launch_bounds__(RM_BLOCK) void rm_flip_check_kernel(NudfMeshTopo a) {
  const int64_t e = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
  if (e >= a.n_edges) return;
  const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1], count = a.edges[5 * e + 2];
  int status = NUDF_REMESH_CANDIDATE;
  int64_t gain = 0, ca = -1, cb = -1;
  Wings w;
  if (count != 2 || u == v || !vertex_ok(a, u) || !vertex_ok(a, v)) {
    status = NUDF_REMESH_COUNT;
  } else if (!wings_of(a, e, &w) || w.ca == w.cb || w.ca == u || w.ca == v || w.cb == u || w.cb == v) {
    status = NUDF_REMESH_SAME;
  } else {
    ca = w.ca, cb = w.cb;
    if (a.sp_sd_vclass[u] > 1 || a.sp_sd_vclass[v] > 1 || a.sp_sd_vclass[ca] > 1 || a.sp_sd_vclass[cb] > 1) {
      status = NUDF_REMESH_CLASS;
    } else if (find_edge(a, (ca < cb ? ca : cb) * a.n_verts + (ca < cb ? cb : ca)) >= 0) {
      status = NUDF_REMESH_EXISTS;
    } else {
      gain = (deviation2(a, u, 0) + deviation2(a, v, 0) + deviation2(a, ca, 0) + deviation2(a, cb, 0)) -
             (deviation2(a, u, -1) + deviation2(a, v, -1) + deviation2(a, ca, 1) + deviation2(a, cb, 1));
      if (!(gain > 0)) {
        status = NUDF_REMESH_GAIN;
      } else {
        const int64_t *t0 = a.faces + w.h0 / 3 * 3, *t1 = a.faces + w.h1 / 3 * 3;
        const V3 none = {0.0, 0.0, 0.0};
        const V3 n0 = normal_of(a, t0[0], t0[1], t0[2], -1, -1, none), n1 = normal_of(a, t1[0], t1[1], t1[2], -1, -1, none);
        const V3 m0 = normal_of(a, t0[0] == v ? cb : t0[0], t0[1] == v ? cb : t0[1], t0[2] == v ? cb : t0[2], -1, -1, none);
        const V3 m1 = normal_of(a, t1[0] == u ? ca : t1[0], t1[1] == u ? ca : t1[1], t1[2] == u ? ca : t1[2], -1, -1, none);
        const bool alike = (a.faces[w.h0] == u) != (a.faces[w.h1] == u);            // the half-edges run against each other
        const double x01 = vdot(m0, n1), x10 = vdot(m1, n0);
        if (!(vdot(m0, n0) > 0.0 && vdot(m1, n1) > 0.0 && (alike ? x01 : -x01) > 0.0 && (alike ? x10 : -x10) > 0.0))
          status = NUDF_REMESH_FOLD;
      }
    }
  }
  a.sp_sd_hf_rm_status[e] = (uint8_t)status;
  a.sp_sd_hf_rm_gain[e] = (int32_t)gain;
  a.sp_sd_hf_rm_ab[2 * e] = ca;
  a.sp_sd_hf_rm_ab[2 * e + 1] = cb;
}

// ---- (e) the winning flips -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_BLOCK) void rm_flip_apply_kernel(NudfMeshTopo a) {
  const int64_t e = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
  if (e >= a.n_edges) return;
  uint8_t win = 0;
  const int64_t u = a.edges[5 * e], v = a.edges[5 * e + 1], r = rank_of(a, e);
  const int64_t ca = a.sp_sd_hf_rm_ab[2 * e], cb = a.sp_sd_hf_rm_ab[2 * e + 1];
  Wings w;
  if (r < a.n_edges && vertex_ok(a, u) && vertex_ok(a, v) && vertex_ok(a, ca) && vertex_ok(a, cb) && a.edges[5 * e + 2] == 2 &&
      wings_of(a, e, &w) && w.ca == ca && w.cb == cb && r == a.sp_sd_hf_rm_best_in[u] && r == a.sp_sd_hf_rm_best_in[v] &&
      r == a.sp_sd_hf_rm_best_in[ca] && r == a.sp_sd_hf_rm_best_in[cb]) {
    win = 1;
    const int64_t f0 = w.h0 / 3, f1 = w.h1 / 3;
    for (int k = 0; k < 3; ++k) {
      const int64_t x = a.faces[3 * f0 + k], y = a.faces[3 * f1 + k];
      a.sp_sd_hf_rm_faces_out[3 * f0 + k] = x == v ? cb : x;
      a.sp_sd_hf_rm_faces_out[3 * f1 + k] = y == u ? ca : y;
    }
  }
  a.sp_sd_hf_rm_win[e] = win;
}

// ---- (f) the tangential relaxation ------------------------------------------------------------------------------------------
// the corner of face f that is neither w nor x, or -1
__device__ __forceinline__ int64_t third_vertex(const NudfMeshTopo& a, int64_t f, int64_t w, int64_t x) {
  if (f < 0 || f >= a.n_faces) return -1;
  const int64_t* t = a.faces + 3 * f;
  for (int k = 0; k < 3; ++k)
    if (t[k] != w && t[k] != x) return vertex_ok(a, t[k]) ? t[k] : -1;
  return -1;
}

struct Normal {
  V3 sum, first;
  bool have;
};

// adds (p_x - p_w) x (p_y - p_w) with the sign that agrees with the first one taken
__device__ __forceinline__ void add_wedge(const NudfMeshTopo& a, const V3& pw, const V3& ex, int64_t y, Normal* N) {
  if (y < 0) return;
  const V3 n = vcross(ex, vsub(vload(a.pos + 3 * y), pw));
  if (!positive_finite(dot3(n.x, n.y, n.z))) return;
  if (!N->have) {
    N->sum = N->first = n;
    N->have = true;
  } else if (vdot(n, N->first) >= 0.0) {
    N->sum = {add(N->sum.x, n.x), add(N->sum.y, n.y), add(N->sum.z, n.z)};
  } else {
    N->sum = {sub(N->sum.x, n.x), sub(N->sum.y, n.y), sub(N->sum.z, n.z)};
  }
}

__global__ __launch_bounds__(RM_BLOCK) void rm_relax_kernel(NudfMeshTopo a) {
  const int64_t w = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
  if (w >= a.n_verts) return;
  const V3 p = vload(a.pos + 3 * w);
  double* o = a.sp_sd_hf_rm_pos_out + 3 * w;
  o[0] = p.x, o[1] = p.y, o[2] = p.z;
  int64_t b, e, eb, ee;
  if (a.sp_sd_vclass[w] != 0 || !csr_range(a.sp_sd_ring_off, w, a.sp_sd_n_ring, &b, &e) || e <= b ||
      !csr_range(a.sp_sd_hf_rm_vedge_off, w, a.sp_sd_hf_rm_n_vedge, &eb, &ee))
    return;
  for (int64_t j = b; j < e; ++j)
    if (!vertex_ok(a, a.sp_sd_ring[j])) return;
  V3 s = vload(a.pos + 3 * a.sp_sd_ring[b]);
  for (int64_t j = b + 1; j < e; ++j) {
    const double* r = a.pos + 3 * a.sp_sd_ring[j];
    s = {add(s.x, r[0]), add(s.y, r[1]), add(s.z, r[2])};
  }
  const double nd = (double)(e - b);
  const V3 q = {__ddiv_rn(s.x, nd), __ddiv_rn(s.y, nd), __ddiv_rn(s.z, nd)};
  Normal N = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, false};
  for (int64_t j = eb; j < ee; ++j) {
    const int64_t g = a.sp_sd_hf_rm_vedge[j];
    if (g < 0 || g >= a.n_edges) continue;
    const int64_t* row = a.edges + 5 * g;
    const int64_t x = row[0] == w ? row[1] : row[0];
    if (x == w || !vertex_ok(a, x) || (row[0] != w && row[1] != w)) continue;
    const int64_t y0 = third_vertex(a, row[3], w, x), y1 = row[2] >= 2 ? third_vertex(a, row[4], w, x) : -1;
    const V3 ex = vsub(vload(a.pos + 3 * x), p);
    const bool swap = y0 >= 0 && y1 >= 0 && y1 < y0;
    add_wedge(a, p, ex, swap ? y1 : y0, &N);
    add_wedge(a, p, ex, swap ? y0 : y1, &N);
  }
  const double len2 = dot3(N.sum.x, N.sum.y, N.sum.z);
  if (!N.have || !positive_finite(len2)) return;
  const double len = __dsqrt_rn(len2);
  const V3 nh = {__ddiv_rn(N.sum.x, len), __ddiv_rn(N.sum.y, len), __ddiv_rn(N.sum.z, len)};
  const double d = vdot(vsub(p, q), nh);
  o[0] = add(q.x, mul(d, nh.x));
  o[1] = add(q.y, mul(d, nh.y));
  o[2] = add(q.z, mul(d, nh.z));
}

// ---- launchers --------------------------------------------------------------------------------------------------------
// the counts every entry point is handed; NULL when they are in order, else what is wrong
static const char* bad_sizes(const NudfMeshTopo& a) {
  const int64_t lim = 1LL << 31;
  if (a.n_faces < 0 || a.n_faces >= lim) return "n_faces must be in [0, 2^31)";
  if (a.n_verts < 0 || a.n_verts >= lim) return "n_verts must be in [0, 2^31)";
  if (a.n_edges < 0 || a.n_edges > 3 * a.n_faces) return "n_edges must be in [0, 3 n_faces]";
  if (a.sp_sd_n_ring < 0) return "sp_sd_n_ring must be >= 0";
  if (a.sp_sd_n_border < 0) return "sp_sd_n_border must be >= 0";
  if (a.sp_sd_hf_rm_n_vedge < 0) return "sp_sd_hf_rm_n_vedge must be >= 0";
  return nullptr;
}

static bool no_ring(const NudfMeshTopo& a) { return !a.sp_sd_ring_off || (a.sp_sd_n_ring > 0 && !a.sp_sd_ring); }
static bool no_vedge(const NudfMeshTopo& a) { return !a.sp_sd_hf_rm_vedge_off || (a.sp_sd_hf_rm_n_vedge > 0 && !a.sp_sd_hf_rm_vedge); }
static bool no_corners(const NudfMeshTopo& a) { return !a.sp_sd_hf_rm_corner_off || !a.sp_sd_hf_rm_corner; }

extern "C" int nudf_meshremesh_collapse_check(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshremesh_collapse_check";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_edges <= 0) return 0;
  if (!positive_finite(a.sp_sd_hf_rm_low)) return refuse(entry, "sp_sd_hf_rm_low must be positive and finite");
  if (!positive_finite(a.sp_sd_hf_rm_high)) return refuse(entry, "sp_sd_hf_rm_high must be positive and finite");
  if (!(a.sp_sd_hf_rm_cos_border >= -1.0 && a.sp_sd_hf_rm_cos_border <= 1.0))
    return refuse(entry, "sp_sd_hf_rm_cos_border must be in [-1, 1]");
  if (!a.faces || !a.edges || !a.he_id || !a.edge_start || !a.pos || !a.sp_sd_vclass || !a.nbr_off || (a.sp_sd_n_border > 0 && !a.nbr) ||
      no_ring(a) || no_corners(a) || !a.sp_sd_hf_rm_status || !a.sp_sd_hf_rm_keep || !a.sp_sd_hf_rm_gone)
    return refuse(entry, "NULL faces, edges, he_id, edge_start, pos, sp_sd_vclass, nbr_off, nbr, sp_sd_ring_off, sp_sd_ring, "
                         "sp_sd_hf_rm_corner_off, sp_sd_hf_rm_corner, sp_sd_hf_rm_status, sp_sd_hf_rm_keep or sp_sd_hf_rm_gone");
  MESH_LAUNCH(rm_collapse_check_kernel, a.n_edges, RM_BLOCK, RM_BLOCK, entry);
}

extern "C" int nudf_meshremesh_vertex_min(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshremesh_vertex_min";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_verts <= 0) return 0;
  if (a.sp_sd_hf_rm_mode < 0 || a.sp_sd_hf_rm_mode > 2)
    return refuse(entry, "sp_sd_hf_rm_mode must be 0 (edges at the vertex), 1 (one-ring) or 2 (edges of the faces)");
  if (!a.sp_sd_hf_rm_best_out) return refuse(entry, "NULL sp_sd_hf_rm_best_out");
  if (a.sp_sd_hf_rm_mode == 1) {
    if (!a.sp_sd_hf_rm_best_in || no_ring(a)) return refuse(entry, "NULL sp_sd_hf_rm_best_in, sp_sd_ring_off or sp_sd_ring");
    if (a.sp_sd_hf_rm_best_in == a.sp_sd_hf_rm_best_out) return refuse(entry, "sp_sd_hf_rm_best_in and sp_sd_hf_rm_best_out must differ");
  } else {
    if (a.n_edges > 0 && (!a.sp_sd_hf_rm_status || !a.sp_sd_hf_rm_rank)) return refuse(entry, "NULL sp_sd_hf_rm_status or sp_sd_hf_rm_rank");
    if (a.sp_sd_hf_rm_mode == 0 && no_vedge(a)) return refuse(entry, "NULL sp_sd_hf_rm_vedge_off or sp_sd_hf_rm_vedge");
    if (a.sp_sd_hf_rm_mode == 2 && a.n_faces > 0 && (no_corners(a) || !a.he_edge))
      return refuse(entry, "NULL sp_sd_hf_rm_corner_off, sp_sd_hf_rm_corner or he_edge");
    if (a.sp_sd_hf_rm_mode == 2 && a.n_faces <= 0 && !a.sp_sd_hf_rm_corner_off) return refuse(entry, "NULL sp_sd_hf_rm_corner_off");
  }
  MESH_LAUNCH(rm_vertex_min_kernel, a.n_verts, RM_BLOCK, RM_BLOCK, entry);
}

extern "C" int nudf_meshremesh_collapse_apply(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshremesh_collapse_apply";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_edges <= 0) return 0;
  if (!a.edges || !a.pos || !a.sp_sd_vclass || !a.sp_sd_hf_rm_status || !a.sp_sd_hf_rm_rank || !a.sp_sd_hf_rm_keep || !a.sp_sd_hf_rm_gone ||
      !a.sp_sd_hf_rm_best_in || !a.sp_sd_hf_rm_remap || !a.sp_sd_hf_rm_pos_out || !a.sp_sd_hf_rm_win)
    return refuse(entry, "NULL edges, pos, sp_sd_vclass, sp_sd_hf_rm_status, sp_sd_hf_rm_rank, sp_sd_hf_rm_keep, sp_sd_hf_rm_gone, "
                         "sp_sd_hf_rm_best_in, sp_sd_hf_rm_remap, sp_sd_hf_rm_pos_out or sp_sd_hf_rm_win");
  MESH_LAUNCH(rm_collapse_apply_kernel, a.n_edges, RM_BLOCK, RM_BLOCK, entry);
}

extern "C" int nudf_meshremesh_flip_check(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshremesh_flip_check";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_edges <= 0) return 0;
  if (!a.faces || !a.edges || !a.he_id || !a.edge_start || !a.edge_key || !a.pos || !a.sp_sd_vclass || no_ring(a) ||
      !a.sp_sd_hf_rm_status || !a.sp_sd_hf_rm_gain || !a.sp_sd_hf_rm_ab)
    return refuse(entry, "NULL faces, edges, he_id, edge_start, edge_key, pos, sp_sd_vclass, sp_sd_ring_off, sp_sd_ring, "
                         "sp_sd_hf_rm_status, sp_sd_hf_rm_gain or sp_sd_hf_rm_ab");
  MESH_LAUNCH(rm_flip_check_kernel, a.n_edges, RM_BLOCK, RM_BLOCK, entry);
}

extern "C" int nudf_meshremesh_flip_apply(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshremesh_flip_apply";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_edges <= 0) return 0;
  if (!a.faces || !a.edges || !a.he_id || !a.edge_start || !a.sp_sd_hf_rm_status || !a.sp_sd_hf_rm_rank || !a.sp_sd_hf_rm_ab ||
      !a.sp_sd_hf_rm_best_in || !a.sp_sd_hf_rm_faces_out || !a.sp_sd_hf_rm_win)
    return refuse(entry, "NULL faces, edges, he_id, edge_start, sp_sd_hf_rm_status, sp_sd_hf_rm_rank, sp_sd_hf_rm_ab, "
                         "sp_sd_hf_rm_best_in, sp_sd_hf_rm_faces_out or sp_sd_hf_rm_win");
  MESH_LAUNCH(rm_flip_apply_kernel, a.n_edges, RM_BLOCK, RM_BLOCK, entry);
}

extern "C" int nudf_meshremesh_relax(const NudfMeshTopo* args, void* stream) {
  const NudfMeshTopo& a = *args;
  const char* const entry = "nudf_meshremesh_relax";
  if (const char* why = bad_sizes(a)) return refuse(entry, why);
  if (a.n_verts <= 0) return 0;
  if (!a.pos || !a.sp_sd_hf_rm_pos_out || !a.sp_sd_vclass || no_ring(a) || no_vedge(a) || (a.n_edges > 0 && !a.edges) ||
      (a.n_faces > 0 && !a.faces))
    return refuse(entry, "NULL pos, sp_sd_hf_rm_pos_out, sp_sd_vclass, sp_sd_ring_off, sp_sd_ring, sp_sd_hf_rm_vedge_off, "
                         "sp_sd_hf_rm_vedge, edges or faces");
  MESH_LAUNCH(rm_relax_kernel, a.n_verts, RM_BLOCK, RM_BLOCK, entry);
}
