// Level-set marching cubes of a scalar grid (include/nudf.h NudfIsoSurface, NudfIsoSurfaceSparse): the surface
// {F = level} of a signed or unsigned field, what the reference gets from PyMCubes in extract_geometry.  The dense and
// the sparse pipeline of mc_pipeline.h under McLevelRule over the MeshUDF mesher's case table: corner c of a cell is `-`
// iff F_c < level, a cell with a non-finite corner emits nothing, and the vertex of an edge lies at the linear
// interpolation clamped to the edge (isosurface_cell.h).  The ordering contract is the MeshUDF mesher's.
#include "mc_pipeline.h"

__device__ __forceinline__ const float* mc_field(const NudfIsoSurface& a) { return a.F; }
__device__ __forceinline__ const float* mc_field(const NudfIsoSurfaceSparse& a) { return a.F; }

MC_DENSE_ENTRY(nudf_isosurface_classify, NudfIsoSurface, mc_dense_cells(a), mc_dense_classify_kernel<McLevelRule, NudfIsoSurface>)
MC_DENSE_ENTRY(nudf_isosurface_emit, NudfIsoSurface, a.n_cells, mc_dense_emit_kernel<NudfIsoSurface>)
MC_DENSE_ENTRY(nudf_isosurface_vertices, NudfIsoSurface, a.n_edges, mc_dense_vertices_kernel<McLevelRule, NudfIsoSurface>)

MC_SPARSE_CLASSIFY_ENTRY(nudf_isosurface_sparse_classify, NudfIsoSurfaceSparse, McLevelRule)
MC_SPARSE_ENTRY(nudf_isosurface_sparse_edges, NudfIsoSurfaceSparse, a.n_cells, mc_sparse_edges_kernel<NudfIsoSurfaceSparse>)
MC_SPARSE_ENTRY(nudf_isosurface_sparse_emit, NudfIsoSurfaceSparse, a.n_cells, mc_sparse_emit_kernel<NudfIsoSurfaceSparse>)
MC_SPARSE_ENTRY(nudf_isosurface_sparse_vertices, NudfIsoSurfaceSparse, a.n_edges,
                mc_sparse_vertices_kernel<McLevelRule, NudfIsoSurfaceSparse>)
