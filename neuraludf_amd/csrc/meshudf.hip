// MeshUDF open-surface extraction from a dense UDF grid (include/nudf.h NudfMeshUDF): the per-cell and per-edge work of
// the mesher the reference runs serially in Cython (custom_mc udf_mc_lewiner, called by extract_mesh.get_mesh_udf_fast).
// The dense pipeline of mc_pipeline.h under McUdfRule: signs are chosen per cell from the gradients with no propagation
// between cells (meshudf_cell.h), so every cell is independent; the vertex of an edge lies at t = U_a / (U_a + U_b) from
// its lower end.
#include "mc_pipeline.h"

__device__ __forceinline__ const float* mc_field(const NudfMeshUDF& a) { return a.U; }

MC_DENSE_ENTRY(nudf_meshudf_classify, NudfMeshUDF, mc_dense_cells(a), mc_dense_classify_kernel<McUdfRule, NudfMeshUDF>)
MC_DENSE_ENTRY(nudf_meshudf_emit, NudfMeshUDF, a.n_cells, mc_dense_emit_kernel<NudfMeshUDF>)
MC_DENSE_ENTRY(nudf_meshudf_vertices, NudfMeshUDF, a.n_edges, mc_dense_vertices_kernel<McUdfRule, NudfMeshUDF>)
