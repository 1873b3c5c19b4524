// Sparse MeshUDF extraction (include/nudf.h NudfMeshUDFSparse): the dense mesher's cells and edges (meshudf.hip) over the
// bricks of the selected B^3-cell blocks only.  The sparse pipeline of mc_pipeline.h under McUdfRule: G is stored in
// bricks like U and is read from memory in active cells only.  No dense N^3 array.
#include "mc_pipeline.h"

__device__ __forceinline__ const float* mc_field(const NudfMeshUDFSparse& a) { return a.U; }

MC_SPARSE_CLASSIFY_ENTRY(nudf_meshudf_sparse_classify, NudfMeshUDFSparse, McUdfRule)
MC_SPARSE_ENTRY(nudf_meshudf_sparse_edges, NudfMeshUDFSparse, a.n_cells, mc_sparse_edges_kernel<NudfMeshUDFSparse>)
MC_SPARSE_ENTRY(nudf_meshudf_sparse_emit, NudfMeshUDFSparse, a.n_cells, mc_sparse_emit_kernel<NudfMeshUDFSparse>)
MC_SPARSE_ENTRY(nudf_meshudf_sparse_vertices, NudfMeshUDFSparse, a.n_edges,
                mc_sparse_vertices_kernel<McUdfRule, NudfMeshUDFSparse>)
