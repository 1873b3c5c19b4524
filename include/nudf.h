/* libnudf -- C ABI of the MI355X-native NeuralUDF volume-rendering hot path.
 *
 * Plain pointers and sizes only (no torch types).  All pointers are DEVICE pointers to
 * contiguous fp32 unless noted; the caller owns every buffer (kernels never allocate);
 * every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant,
 * and returns 0 or a hipError_t value (text via nudf_last_error()).  No host syncs.
 *
 * Each entry point names the chain of PyTorch ops of the reference (xxlong0/NeuralUDF,
 * paths relative to the reference root) that it replaces -- the reference itself has no
 * native kernels and no FFI; INTEGRATION.md shows the ctypes binding a maintainer adds.
 */
#ifndef NUDF_H
#define NUDF_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ABI version.  Every change to an argument struct, an enum value, a #define or an entry point's signature raises it; a
 * caller that mirrors this header by hand (neuraludf_amd/_lib.py) refuses a library whose nudf_version() differs.
 *   111: nudf_pc_tribin_count / nudf_pc_tribin_emit / nudf_pc_closest (point-to-mesh distance); NudfPointCloud grows by the
 *        md_ fields, appended at its end.  (nudf_pc_raycast and its md_ray_o ... md_count fields were appended later under
 *        the same number: the size table below refuses a package and a library that disagree on the struct's size;
 *        nudf_meshsmooth_* and the sm_ fields at the end of NudfMeshOrient likewise, and nudf_meshsubdiv_* with the sp_sd_
 *        fields at the end of NudfMeshTopo, and nudf_meshhole_* with the sp_sd_hf_ fields after those and the new
 *        NUDF_HOLE_ constants, and nudf_meshremesh_* with the sp_sd_hf_rm_ fields after those and the NUDF_REMESH_
 *        constants: the version stays 111)
 *   110: nudf_meshsimplify_* (mesh simplification); NudfMeshTopo grows by the sp_ fields and n_clusters, appended at its end
 *   109: nudf_abi_struct (below) replaces the per-struct size exports and the step-count export that 108 had collected
 *        instead of version steps: the 20 steps of NudfChain (NUDF_CH_MAX_STEPS), NudfMeshUDFSparse, NudfIsoSurface,
 *        NudfIsoSurfaceSparse, NudfMeshOrient, NudfMeshRaster and the two dispatch reports nudf_mlp_chain_plan /
 *        nudf_gemm_tn_grouped_kernel
 *   108: nudf_meshtopo_* + NudfMeshTopo (mesh clean-up)
 *   107: nudf_pc_* + NudfPointCloud (Chamfer evaluation)
 *   106: nudf_meshudf_* + NudfMeshUDF
 *   105: NudfChain.tile_scale / tile_amax_in / tile_amax_out
 *   104: NudfChain.absmax_out, NudfGemmTNGroup.amax_a / amax_b + prec 4 (struct sizes)
 *   103: NudfChainStep.X3 / ldx3, prec 4 chains, NudfPackFrag.dtype 4 */
#define NUDF_ABI_VERSION 111
int nudf_version(void);
/* every argument struct of this header, once, in the order of their definitions */
#define NUDF_ABI_STRUCTS(X) \
  X(NudfGemmNN) X(NudfGemmTN) X(NudfGemmTNProblem) X(NudfGemmTNGroup) X(NudfComposite) X(NudfCompositeGrad) \
  X(NudfUpsample) X(NudfPixelBlend) X(NudfPixelComposite) X(NudfPatchBlend) X(NudfPatchWarp) X(NudfBlendLoss) \
  X(NudfAdamTensor) X(NudfAdamGroup) X(NudfAdam) X(NudfChainStep) X(NudfChain) X(NudfPackFrag) X(NudfPackLayer) \
  X(NudfPackMulti) X(NudfUnpackLayer) X(NudfUnpackMulti) X(NudfRayBatch) X(NudfMeshUDF) X(NudfMeshUDFSparse) \
  X(NudfIsoSurface) X(NudfIsoSurfaceSparse) X(NudfPointCloud) X(NudfMeshTopo) X(NudfMeshOrient) X(NudfMeshRaster)
/* entry i of that list as the library was compiled (host code only): returns sizeof and stores the struct's name in *name
 * (name may be NULL); -1 for an i outside the list.  A caller that passes these structs by reference checks every size
 * after the version (the Python loader refuses a library in which one differs). */
int nudf_abi_struct(int i, const char** name);
const char* nudf_last_error(void);

/* ------------------------------------------------------------------------------------
 * Non-finite status word.  The reference stops on the host when a NaN appears -- sample_pdf's new samples
 * (models/udf_renderer_blending.py:97-101), up_sample_unbias / up_sample_no_occ_aware's (:265-269, :860-864), the eikonal
 * term of render_core (:543-544) -- each a `.cpu()` sync in the middle of a step.  Here the caller hands the library ONE
 * int32 of device memory (zeroed by the caller); nudf_upsample ORs NUDF_STATUS_NONFINITE_SAMPLES into it when a new sample
 * is not finite, nudf_composite_fwd NUDF_STATUS_NONFINITE_RENDER when a ray's composited outputs (weight sum, depth, the two
 * colours) or one of the three renderer scalars / their parameters (inv_s, beta, gamma) are not, and nudf_step_loss_fwd /
 * nudf_blend_loss_fwd (the fused single-process loss launches -- ONLY those: a ray-sharded job forms its loss from all-reduced
 * sums outside the library, and its host loop looks at that scalar itself, neuraludf_amd/train.py Trainer.check_finite)
 * NUDF_STATUS_NONFINITE_LOSS when the step's total loss is not.  (The per-sample alphas and weights themselves cannot leave
 * [0, 1]: the reference's clips are hardware min / max here, which drop a NaN operand -- a NaN network output or parameter
 * therefore shows up in the colours, the scalars and the loss, which is where the bits look.)  Nothing on the device reads the word
 * and no call waits for it: the caller polls it when it likes (UDFRendererBlending.status(), Trainer.iteration every
 * `status_every` iterations).  NULL (the default) switches the checks off.  The pointer is per process (one process per
 * GPU); it is passed to the kernels as an argument, so launches captured in a HIP graph keep the word they were captured with.
 * ---------------------------------------------------------------------------------- */
enum {
  NUDF_STATUS_NONFINITE_RENDER = 1,
  NUDF_STATUS_NONFINITE_SAMPLES = 2,
  NUDF_STATUS_NONFINITE_LOSS = 4
};
int nudf_set_status_flag(int32_t* device_word);
int32_t* nudf_status_flag(void);

/* ------------------------------------------------------------------------------------
 * Dense layer GEMMs (fp32 MFMA).  Replace F.linear + weight_norm + Softplus/ReLU and their
 * autograd (double-)backward:  models/fields.py:192-231 (UDFNetwork.forward/.gradient),
 * :452-495 (ResidualRenderingNetwork.forward), :599-628 (NeRF.forward).
 * ---------------------------------------------------------------------------------- */
enum {
  NUDF_EPI_NONE = 0,      /* C1 = (acc + bias) * scale                                   */
  NUDF_EPI_SOFTPLUS = 1,  /* C1 = softplus100(acc+bias)*scale ; C2 = softplus100'(..)     */
  NUDF_EPI_RELU = 2,      /* C1 = relu(acc+bias)*scale                                   */
  NUDF_EPI_MUL = 3,       /* C1 = acc * X1 * scale                                       */
  NUDF_EPI_MULMASK = 4,   /* C1 = (X1 > 0) ? acc*scale : 0      (ReLU backward)          */
  NUDF_EPI_TANGENT = 5,   /* s from X1 (as MULSP): C1 = acc*s*scale ; C2 = acc*X2*100*(1-s)  */
  NUDF_EPI_BWD = 6,       /* s from X1 (as MULSP): C1 = acc*scale*s + X2                   */
  NUDF_EPI_SIGMOID = 7,   /* cols < iparam: sigmoid -> C1 (and C2) ; others raw -> C3[row, col-iparam] (or C1) */
  NUDF_EPI_UDFHEAD = 8,   /* col 0: |v|*scale -> C2[row], sign -> C3[row]; col c>0 -> C1[row,c-1] */
  NUDF_EPI_SKIPSPLIT = 9, /* col < iparam: C1 = acc*s*scale (s from X1) ; else C2[col-iparam] = acc*scale */
  NUDF_EPI_RELU_DUAL = 10,/* C1 = C2 = relu(acc+bias)                                    */
  NUDF_EPI_ADDMASK = 11,  /* C1 = (X1 > 0) ? (acc + X2)*scale : 0   (ReLU backward at a join) */
  NUDF_EPI_MULSP = 12     /* C1 = acc * softplus'(.) * scale, softplus' recovered from X1 = stored softplus output * (1/xscale) */
};

typedef struct NudfGemmNN {
  const float* A; int32_t lda;      /* [M, K] row-major, K % 32 == 0, lda % 4 == 0        */
  const float* B; int32_t ldb;      /* [K, ldb] row-major (packed W^T or W), ldb % 4 == 0 */
  const float* bias;                /* [N] or NULL                                        */
  float* C1; int32_t ldc1;          /* [M, N]                                             */
  float* C2; int32_t ldc2;          /* second output or NULL                              */
  float* C3; int32_t ldc3;          /* third output (UDFHEAD: sign per row; SIGMOID: raw tail) or NULL */
  const float* X1; int32_t ldx1;    /* epilogue operand 1 [M, N] or NULL                  */
  const float* X2; int32_t ldx2;    /* epilogue operand 2 [M, N] or NULL                  */
  int32_t M, N, K;
  int32_t epi;                      /* NUDF_EPI_*                                         */
  int32_t iparam;
  float scale;
  float xscale;                     /* X1 holds softplus output / xscale (MULSP, TANGENT, BWD, SKIPSPLIT) */
} NudfGemmNN;

/* C[M,N] = epilogue(A[M,K] B[K,N]) */
int nudf_gemm_nn(const NudfGemmNN* args, void* stream);

typedef struct NudfGemmTN {
  const float* A1; int32_t lda1; int32_t na1;   /* [M, na1]                               */
  const float* B1; int32_t ldb1;                /* [M, ldb1]                              */
  const float* A2; int32_t lda2; int32_t na2;   /* optional second pair (NULL to skip)    */
  const float* B2; int32_t ldb2;
  float* C; int32_t ldc;                        /* [NA, NB], accumulated with atomics     */
  float* dbias;                                 /* [NA] += column sums of A1, or NULL     */
  int32_t M, NA, NB;
  int32_t rows_per_block;                       /* 0 = choose                             */
  int32_t prec;                                 /* MFMA operand precision: 0 = fp32 (exact), 2 = bf16 operands converted
                                                   from the fp32 tiles on the fly, fp32 accumulate (config-5 mode),
                                                   3 = bf16x3: fp32 emulated on the bf16 pipe (both operands split exactly
                                                   into three bf16 parts, six products; see NudfChainStep.prec)      */
} NudfGemmTN;

/* C[NA,NB] += A1^T B1 (+ A2^T B2): weight gradients, reduction over the M points */
int nudf_gemm_tn(const NudfGemmTN* args, void* stream);

/* up to 12 single-pair problems over the same M points in one launch (all weight gradients of a layer chain); at most
 * 64 output tiles of 128 x 128 in total.  A1 / B1 16-byte aligned, lda1 / ldb1 multiples of 4. */
#define NUDF_TN_MAX_PROBLEMS 12
typedef struct NudfGemmTNProblem {
  const float* A1; const float* B1;             /* [M, lda1], [M, ldb1]                   */
  float* C; float* dbias;                       /* [NA, ldc] +=, [NA] += or NULL          */
  int32_t lda1, ldb1, ldc, NA, NB;
  int32_t tile_start;                           /* unused (kept for layout compatibility) */
  int32_t flags;                                /* NUDF_TN_A16 / NUDF_TN_B16: that operand is stored as bf16 (leading
                                                   dimension in elements, a multiple of 8); widened to fp32 on chip    */
} NudfGemmTNProblem;
#define NUDF_TN_A16 1
#define NUDF_TN_B16 2
#define NUDF_TN_A_BLK 4                         /* fp32 operand in the BLOCKED layout of NudfChainStep (rows padded to 32) */
#define NUDF_TN_B_BLK 8
#define NUDF_TN_A_P4 16                         /* with NUDF_TN_A16: the bf16 operand is 4-point packed like the chains'
                                                   16-bit stored state (NUDF_CH_STATE16): element (row, col) at
                                                   ((row / 4) ld + col) 4 + row % 4, rows padded to a multiple of 4    */
#define NUDF_TN_B_P4 32
typedef struct NudfGemmTNGroup {
  int32_t n_problems, M, rows_per_block, total_tiles;   /* rows_per_block 0 = choose      */
  int32_t prec;                                 /* as NudfGemmTN.prec; 4 = f16x2 (see amax_a / amax_b below) */
  NudfGemmTNProblem prob[NUDF_TN_MAX_PROBLEMS];
  float* workspace;                             /* NULL: partial tiles are accumulated with fp32 atomics.  Otherwise a
                                                   16-byte aligned scratch of >= nudf_gemm_tn_grouped_workspace()
                                                   floats: every workgroup stores its partial tile there and a second
                                                   kernel adds them to C / dbias in a FIXED order (run-to-run identical
                                                   results).  Must not be shared by launches that can overlap.  With a
                                                   workspace the problems of ONE group must write pairwise disjoint C
                                                   and dbias ranges (that reduction is not atomic; overlapping groups
                                                   are refused with hipErrorInvalidValue); consecutive launches may
                                                   accumulate into the same C.                                       */
  int64_t workspace_floats;
  int32_t assign;                               /* != 0 (workspace path only): the reduction ASSIGNS C and dbias (0 + the
                                                   ordered sum) instead of adding to them -- the first launch into a
                                                   gradient buffer then needs no zero fill.  Elements the group does not
                                                   cover (rows >= NA, columns >= NB) are left untouched.               */
  /* prec 4 (f16x2: three fp16 MFMA products per fp32 product, NudfChainStep.prec 4) only: device scalars holding max |x| over
     ALL A operands / ALL B operands of the group (written by the sweeps that produce them, NudfChain.absmax_out), or NULL for a
     side whose operands lie in fp16's range as they are (activations).  Each side is multiplied by
     2^(10 - floor(log2 max)) before the split and C by the reciprocals afterwards -- exact; a scaled element beyond +-60 000
     (a maximum that was not reported) is clamped. */
  const float* amax_a;
  const float* amax_b;
} NudfGemmTNGroup;
int nudf_gemm_tn_grouped(const NudfGemmTNGroup* args, void* stream);
/* floats of workspace this group needs (0 for an empty group, < 0 on an invalid one) */
int64_t nudf_gemm_tn_grouped_workspace(const NudfGemmTNGroup* args);
/* the launch plan, for tests (host code only): out[4 b ..] = {problem, tile row * 256 + tile column, row chunk, workspace
 * slot} of workgroup b, or {-1, -1, -1, -1} for a HOLE (a workgroup that exits at once); returns the number of workgroups
 * LAUNCHED (at most `capacity` are written), < 0 on an invalid group.  Workgroups b and b' with b % 8 == b' % 8 run on the
 * same XCD: the tiles of a problem that read the same row chunk are given the same b % 8 -- every chunk, the holes are what
 * that costs -- and no XCD receives more live workgroups than it holds at once (64). */
int nudf_gemm_tn_grouped_plan(const NudfGemmTNGroup* args, int32_t* out, int capacity);
/* which kernel nudf_gemm_tn_grouped gives this group (host code only: the launcher's own plan, checks and selection; nothing
 * the group points to is read, nothing is launched).  name (capacity bytes) receives gemm_tn_group_kernel (the generic fp32-image
 * kernel), gemm_tn16_group_kernel, gemm_tn3_group_kernel or gemm_tn2_group_kernel, and out[0..3] =
 * {grid.x, block.x, grid.x of the tn_reduce_kernel launch that follows (workspace path) or 0, 0}.  Returns what
 * nudf_gemm_tn_grouped would return before launching: 0, or the error of a refused group (text in nudf_last_error, empty
 * name, zero grids).  An empty group gives 0, an empty name and zero grids. */
int nudf_gemm_tn_grouped_kernel(const NudfGemmTNGroup* args, char* name, int capacity, int32_t* out);
/* tuning / cross-check bits (every one computes correct results), returns the old value: 8 = ignore the workspace
 * (atomics), 16 = equal row chunks for every tile instead of the cost-weighted split, 32 = no 2 x 2 quadrant layout for full
 * tiles, 64 = tile-major workgroup order instead of the XCD-aware one, 128 = full fp32 tiles through the generic k-loop
 * instead of the interleaved one, 256 = 16-bit MFMA mode (prec != 0) through the generic kernel's fp32 LDS image instead of
 * the packed k-pair image (bit-identical C either way), 512 = bf16x3 mode through the generic kernel (split on the way out of
 * the fp32 image), 2048 = bf16x3 split-image kernel: every k-step through the generic staging.  Bits 2 and 4 (once
 * timing-only: wrong results) and 1024 (the wide bf16x3 kernel: measured slower, deleted) are retired and ignored.
 * Default 0 (env NUDF_TN_FLAGS). */
int nudf_set_tn_flags(int flags);
/* tuning only: device buffer of >= 4 int64 per workgroup receiving {start, end} (wall_clock64, 100 MHz), tile layout * 16
 * + live sub-tiles per wave | CU identity (HW_ID [15:8] << 8, XCC_ID << 32), k-steps | shader-clock ticks of the same
 * span << 16; NULL switches it off */
int nudf_set_tn_debug(void* buf);


/* ------------------------------------------------------------------------------------
 * Fused UDF -> density -> alpha -> composite (forward / backward), one wavefront per ray.
 * Replaces models/udf_renderer_blending.py:352-362, 370-423, 484-553 (+ :151-159, :292-320).
 * ---------------------------------------------------------------------------------- */
typedef struct NudfComposite {
  const float* rays_o; const float* rays_d;   /* [N,3]                                     */
  const float* z;                              /* [N,S] sorted sample positions             */
  const float* udf;                            /* [N,S] unsigned distance at the mid points */
  const float* grad;                           /* [N,S,3] d udf / d x                       */
  const float* color;                          /* [N,S,3] view-dependent colour (sigmoid'd) */
  const float* color_base;                     /* [N,S,3]                                   */
  const float* bg_z;                           /* [N,n_out] outside sample positions / NULL */
  const float* bg_sigma;                       /* [N,n_out] raw NeRF density                */
  const float* bg_color;                       /* [N,n_out,3]                               */
  const float* scal;                           /* [3] device: inv_s, beta, gamma (clipped)  */
  const float* sample_dist;                    /* [1] device                                */
  const float* background_rgb;                 /* [3] device or NULL                        */
  int32_t N, S, n_out, s_nominal;              /* s_nominal: #weights summed into weight_sum */
  int32_t has_anneal; float cos_anneal;        /* cos_anneal_ratio (None -> has_anneal = 0) */
  float flip_saturation;
  int32_t use_norm_grad;
  float sparse_scale;
  int32_t alpha_type;                          /* sdf2alpha_type: 0 'numerical' (every shipped conf), 1 'theorical'
                                                  (udf_renderer_blending.py:321-323); occupies what was padding   */
  /* outputs */
  float* weights;                              /* [N,S+n_out]                               */
  float* out_color; float* out_color_base;     /* [N,3]                                     */
  float* out_depth;                            /* [N]                                       */
  float* out_normals;                          /* [N,3]                                     */
  float* out_wsum; float* out_wsum_all;        /* [N]                                       */
  float* sums;                                 /* [5] {eik_num, eik_den, eikns_num, eikns_den, sparse_sum}: assigned when ws is
                                                  given, += (caller zeroes) on the atomic path */
  float* ws;                                   /* scratch [5 * ceil(N/4)] for per-block partial sums (two-stage,
                                                  deterministic; NULL = one atomic per block and sum, which serialises
                                                  at the memory side for large N) */
  /* optional diagnostics, [N,S] each or NULL */
  float* o_alpha; float* o_alpha_plus; float* o_alpha_minus; float* o_vis_prob;
  float* o_alpha_occ; float* o_raw_occ; float* o_true_cos; float* o_grad_mag;
  float* o_mid_z; float* o_dists; float* o_inside; float* o_flip;
  const float* sched;                          /* [2] device {cos_anneal_ratio, flip_saturation} overriding the two by-value
                                                  fields above, or NULL: lets a captured HIP graph of the train step (kernel
                                                  arguments frozen at capture) follow the per-iteration schedules
                                                  (exp_runner_blending.py:193-228); has_anneal stays by value            */
  /* the renderer scalars formed in this launch instead of by nudf_scalars_fwd (one launch less each way):
     p_variance != NULL -> `scal` is ignored; inv_s / beta / gamma come from the three 1-element parameters exactly as
     nudf_scalars_fwd forms them (beta_hi = 1 / beta_min), and the forward writes them to scal_out [3] / recip_out [2]
     (= 1 / inv_s, 1 / beta) when given */
  const float* p_variance; const float* p_beta; const float* p_gamma;
  float beta_hi;
  int32_t defer_sums;                          /* != 0 (needs ws): the per-block partials stay in ws and `sums` is NOT
                                                  written -- nudf_partial_sums(ws, ceil(N/4), 5, sums) or the ws argument
                                                  of nudf_step_loss_fwd finishes the reduction in the consumer's launch */
  float* scal_out; float* recip_out;
} NudfComposite;

typedef struct NudfCompositeGrad {
  /* upstream (any may be NULL = zero) */
  const float* d_color; const float* d_color_base;   /* [N,3]                              */
  const float* d_weights;                             /* [N,S+n_out]                        */
  const float* d_depth;                               /* [N]                                */
  const float* d_normals;                             /* [N,3]                              */
  const float* d_wsum; const float* d_wsum_all;       /* [N]                                */
  const float* d_sums;                                /* [5] device                         */
  /* results */
  float* o_d_udf;                                     /* [N,S]                              */
  float* o_d_grad;                                    /* [N,S,3]                            */
  float* o_d_color; float* o_d_color_base;            /* [N,S,3] or NULL                    */
  float* o_d_bg_sigma;                                /* [N,n_out] or NULL                  */
  float* o_d_bg_color;                                /* [N,n_out,3] or NULL                */
  float* o_d_scal;                                    /* [3] d inv_s, d beta, d gamma: assigned when ws is given, += otherwise */
  float* ws;                                          /* scratch [3 * ceil(N/4)] or NULL (see NudfComposite.ws) */
  float* o_d_param;                                   /* [3] d variance, d beta, d gamma (needs p_variance and ws): the
                                                         reduction of the partials and nudf_scalars_bwd as one launch */
} NudfCompositeGrad;

int nudf_composite_fwd(const NudfComposite* args, void* stream);
int nudf_composite_bwd(const NudfComposite* args, const NudfCompositeGrad* grads, void* stream);
/* out[k] = sum over the nblk rows of ws [nblk, K] (K <= 8), fixed order: the second stage of the composite kernels'
 * deterministic batch sums, for a caller that asked them to leave the partials (NudfComposite.defer_sums) */
int nudf_partial_sums(const float* ws, int nblk, int K, float* out, void* stream);
/* per-ray colours from the per-32-point partial sums a colour chain left (NudfChainStep.row_sums [N S / 32, 4]):
 * out[ray][c] = sum of the ray's S / 32 blocks (+ background_rgb[c] (1 - wsum_all[ray]) for `out_color`, :527-528).
 * NudfComposite.color == NULL makes nudf_composite_fwd compute everything BUT the two colour sums (weights first). */
int nudf_composite_colour_finish(const float* sums_color, const float* sums_color_base, int N, int S,
                                 const float* background_rgb, const float* wsum_all, float* out_color,
                                 float* out_color_base, void* stream);

/* ------------------------------------------------------------------------------------
 * Hierarchical importance re-sampling (no autograd), one wavefront per ray.
 *   nudf_upsample: up_sample_unbias (mode 0, models/udf_renderer_blending.py:197-272) or
 *                  up_sample_no_occ_aware (mode 1, :834-866) fused with sample_pdf(det=True) (:66-104)
 *   nudf_merge   : sorted merge of cat_z_vals (:278-288), carrying udf along (udf* may be NULL)
 * ---------------------------------------------------------------------------------- */
typedef struct NudfUpsample {
  const float* rays_o; const float* rays_d;   /* [N,3]                                     */
  const float* z; const float* udf;           /* [N,M] current samples and their udf       */
  const float* u;                              /* [K] quantiles linspace(.5/K, 1-.5/K, K)   */
  const float* sample_dist;                    /* [1] device                                */
  const float* gamma_dev;                      /* [1] device gamma (mix schedule) or NULL   */
  int32_t N, M, K, mode;                       /* mode & 0xff: 0 up_sample_unbias, 1 up_sample_no_occ_aware;
                                                  | NUDF_UP_THEORICAL: sdf2alpha_type 'theorical' in up_sample_unbias
                                                  | NUDF_UP_SERIAL | NUDF_UP_NOCONTRACT: see below */
  float inv_s, beta, gamma;
  float* z_new;                                /* [N,K] ascending                           */
  float* pts_new;                              /* [N*K,3] o + d*z_new, or NULL              */
  float* dbg;                                  /* NULL, or [N, NUDF_UP_DBG_ROWS, M]: the intermediates of up_sample_unbias per
                                                  section -- rows cos_val, vis_prob, alpha_plus, alpha_minus, alpha, weights
                                                  (before sample_pdf's + 1e-5), cdf -- for the stage-wise comparison with the
                                                  reference's tensors (scripts/upsample_first_diff.py); mode 0 only */
  /* the PREVIOUS round's merge (nudf_merge) folded into this launch: merge_K > 0 -> the current samples are the sorted
     merge of prev_z / prev_udf [N, M - merge_K] with add_z / add_udf [N, merge_K]; z / udf above are ignored, the merged
     lists are also written to z_merged / udf_merged [N, M] (same values as nudf_merge writes: data movement only) */
  const float* prev_z; const float* prev_udf;
  const float* add_z; const float* add_udf;
  float* z_merged; float* udf_merged;
  int32_t merge_K;
} NudfUpsample;
#define NUDF_UP_DBG_ROWS 7
#define NUDF_UP_THEORICAL 256
#define NUDF_UP_SERIAL 512      /* the three scans in torch-CPU order: one running DOUBLE accumulator per row, every output
                                   rounded to float (cumprod / cumsum of a float tensor on the CPU); default: wave-parallel
                                   fp32 scans (what the same torch ops do on a GPU) */
#define NUDF_UP_NOCONTRACT 1024 /* kernel build without floating-point contraction: every product / sum of the reference's
                                   op chain rounded separately, as separate torch ops round them */
#define NUDF_UP_SLEEF 2048      /* sigmoid as torch's CPU kernel forms it: 1 / (1 + exp(-x)) with a true division and
                                   Vectorized<float>::exp = Sleef expf u10 (Cody-Waite ln 2 split, degree-5 polynomial in FMAs,
                                   two-step ldexp), restated bit for bit (scripts/sleef_expf_check.py: 1 of 4.5 M sigmoids
                                   differs from torch's on an AVX-512 host).  torch.exp itself goes through MKL's vsExp on
                                   contiguous tensors and is NOT covered: those call sites keep libm's expf */
#define NUDF_UP_EXPCR 4096      /* the exp call sites (udf2logistic, alpha_occ: torch.exp = MKL vsExp HA on the CPU) evaluated in
                                   double and rounded once: the correctly rounded value, which MKL's result equals on 98.9 % of
                                   arguments; default: libm expf */
int nudf_upsample(const NudfUpsample* args, void* stream);
int nudf_merge(const float* z, const float* udf, const float* z_new, const float* udf_new, int N, int M,
               int K, float* z_out, float* udf_out, void* stream);
/* the LAST merge of the schedule (z only, :278-288) + the section mid points the renderer evaluates next
 * (nudf_ray_points mode 1, :352-357) in one launch: z_out [N, M + K], pts [N (M + K), 3].  xrows != NULL: the points are
 * also written to columns 0..2 of the [N (M + K), ldx] row array at xrows and columns 3..xcols-1 are zeroed -- the
 * [feat | pts | 0] input buffer of the colour network (what nudf_copy_cols + a pad fill did).  Same arithmetic as the
 * separate launches. */
int nudf_merge_points(const float* z, const float* z_new, int N, int M, int K, float* z_out, const float* rays_o,
                      const float* rays_d, const float* sample_dist, float* pts, float* xrows, int ldx, int xcols,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * Pixel / patch blending and the SSIM patch loss (gradients reach the blending logits and the
 * compositing weights only, as in the reference).
 * ---------------------------------------------------------------------------------- */
typedef struct NudfPixelBlend {   /* patch_projector.py:21-43, projector_utils.py:8-85, fields.py:498-519 */
  const float* pts;               /* [P,3] sample points                                    */
  const float* logits; int32_t nl;/* [P,nl] blending logits (first V columns used)          */
  const float* proj;              /* [V,12] row-major 3x4 = K_v[:3,:3] @ w2c_v[:3,:]        */
  const float* imgs;              /* [V,3,H,W] source images (img_layout 0) or [V,H,W,3] (img_layout 1) */
  int32_t P, V, H, W;
  float* pix;                     /* [P,3] blended pixel colour per sample                  */
  int32_t img_layout;             /* 1: channel-interleaved texels = the memory behind the reference's
                                     images[src_idx].permute(0,3,1,2) view (dataset.py:147-149); one 12-byte load
                                     per texel instead of three plane loads                              */
} NudfPixelBlend;
int nudf_pixel_blend_fwd(const NudfPixelBlend* a, void* stream);
int nudf_pixel_blend_bwd(const NudfPixelBlend* a, const float* d_pix, float* d_logits, void* stream);

typedef struct NudfPixelComposite {   /* udf_renderer_blending.py:503-518 */
  const float* w;                 /* [N,S+n_out] compositing weights                        */
  const float* pix;               /* [N,S,3]                                                */
  const float* pts;               /* [N,S,3] (inside-sphere test), used when bg_in != NULL  */
  const float* bg_in;             /* [N,S,3] background colour at the inside samples / NULL */
  const float* bg_tail;           /* [N,n_out,3] / NULL                                     */
  int32_t N, S, n_out;
  float* out;                     /* [N,3]                                                  */
} NudfPixelComposite;
int nudf_pixel_composite_fwd(const NudfPixelComposite* a, void* stream);
int nudf_pixel_composite_bwd(const NudfPixelComposite* a, const float* d_out, float* d_w, float* d_pix,
                             float* d_bg_in, float* d_bg_tail, void* stream);

typedef struct NudfPatchBlend {   /* patch_projector.py:45-164, fields.py:521-535, udf_renderer_blending.py:520-524 */
  const float* pts;               /* [N,S,3]                                                */
  const float* grad;              /* [N,S,3] d udf/dx (normal = flip * grad/(|grad|+1e-5))  */
  const float* rays_d;            /* [N,3]                                                  */
  const float* uv;                /* [N,2] ray pixel in the reference image (pixel units)   */
  const float* logits; int32_t nl;/* [N,S,nl]                                               */
  const float* w; int32_t ldw;    /* [N,ldw] compositing weights (first S used)             */
  const float* ref_cam;           /* [24] K_ref^-1 | R_ref | t_ref | cam centre             */
  const float* src_cam;           /* [V,24] K_src | R_rel | t_rel | -R_rel^T t_rel          */
  const float* imgs;              /* [V,3,H,W] (img_layout 0) or [V,H,W,3] (img_layout 1)     */
  int32_t N, S, V, H, W, hps;
  float* patch_colors;            /* [N,(2h+1)^2,3]                                         */
  float* patch_mask;              /* [N] = sum_s w_s [any view sees the whole patch]        */
  int32_t img_layout;             /* as in NudfPixelBlend                                   */
} NudfPatchBlend;
int nudf_patch_blend_fwd(const NudfPatchBlend* a, void* stream);
int nudf_patch_blend_bwd(const NudfPatchBlend* a, const float* d_patch, float* d_logits, float* d_w, void* stream);

/* Un-fused warps = the reference's projector interface itself (PatchProjector.pixel_warp / .patch_warp,
 * models/patch_projector.py:21-43, 45-164): per-VIEW samples and validity masks, forward only (the reference builds
 * the homographies under no_grad and the sample positions carry no gradient to any parameter).  The training path
 * uses the fused kernels above and never materialises these tensors. */
int nudf_pixel_warp(const NudfPixelBlend* a /* logits, pix unused */, float* colors /* [P,V,3] */,
                    float* mask /* [P,V] 0/1 */, void* stream);
typedef struct NudfPatchWarp {
  const float* pts;               /* [N,S,3]                                                */
  const float* normals;           /* [N,S,3] plane normals in world space                   */
  const float* uv;                /* [N,2] ray pixel in the reference image (pixel units)   */
  const float* ref_cam;           /* [24], as in NudfPatchBlend                             */
  const float* src_cam;           /* [V,24]                                                 */
  const float* imgs;              /* [V,3,H,W] (img_layout 0) or [V,H,W,3] (img_layout 1)   */
  int32_t N, S, V, H, W, hps, img_layout;
  float* colors;                  /* [N,S,V,(2h+1)^2,3]                                     */
  float* mask;                    /* [N,S,V,(2h+1)^2] 0/1                                   */
} NudfPatchWarp;
int nudf_patch_warp(const NudfPatchWarp* a, void* stream);

/* loss/patch_metric.py:21-41, 76-84; d_out/d_pred NULL = forward only */
int nudf_ssim_patch(const float* pred, const float* gt, const float* window, int N, int Npx, float* out,
                    const float* d_out, float* d_pred, void* stream);
/* every patch error of ColorPatchLoss (loss/loss.py:66-73, loss/patch_metric.py:44-67): type 0 'ssim', 1 'l1', 2 'ssd',
 * 3 'ncc' (returned as 1 - ncc); pred / gt [N, Npx, 3], window [Npx] (Gaussian, used by ssim / ncc), out [N] */
int nudf_patch_metric(int type, const float* pred, const float* gt, const float* window, int N, int Npx, float* out,
                      const float* d_out, float* d_pred, void* stream);

/* ------------------------------------------------------------------------------------
 * The BLENDING step's loss (BASELINE config 3) in three launches around the caller's sort: ColorLoss with its pixel and
 * trimmed patch terms (loss/loss.py:105-133, :21-44, :66-84), the patch-mask algebra of the runner
 * (exp_runner_blending.py:313-315), the three regularisers from the composite sums and the weighted total (:330-371).
 *   nudf_blend_loss_prepare: m[i] = ((patch_mask[i] * (weight_sum[i] > 0.5)) > 0) as 0 / 1, err_masked[i] = err[i] m[i]
 *   caller: err_sorted, order = sort(err_masked, descending)   (the trimmed mean needs order statistics)
 *   nudf_blend_loss_fwd:     out[12] = {total, colour total, Lb, Lc, Lpix, Lpatch, gradient_error, gradient_error_near_surface,
 *                            sparse_error, den_pix, k = floor(trim_ratio * sum m), kept count}
 *   nudf_blend_loss_bwd:     d cb, d c, d pix [3 N], d err [N] (through the sort's permutation), d sums [5]
 * The weights are read from the device vector w_dev (NUDF_LW_*).  ORs NUDF_STATUS_NONFINITE_LOSS like nudf_step_loss_fwd.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfBlendLoss {
  const float* cb; const float* c; const float* pix; const float* gt;   /* [N,3]                                     */
  const float* err;            /* [N] per-ray patch error (nudf_patch_metric)                                        */
  const float* patch_mask;     /* [N] the renderer's patch validity weight (render result 'patch_mask')              */
  const float* weight_sum;     /* [N]                                                                                */
  const float* err_sorted;     /* [N] descending sort of err_masked (fwd / bwd)                                      */
  const int64_t* order;        /* [N] its permutation                                                                */
  float* m;                    /* [N] prepare: out; fwd / bwd: in                                                     */
  float* err_masked;           /* [N] prepare: out                                                                   */
  float* sums;                 /* [5] composite sums: read -- or, with sums_ws, reduced here and written              */
  const float* sums_ws;        /* NULL, or the composite launch's per-block partials (NudfComposite.defer_sums)      */
  const float* w_dev;          /* [NUDF_LW_COUNT] device                                                             */
  float* out;                  /* [12] fwd: out; bwd: in                                                             */
  const float* d_total;        /* bwd: device scalar upstream gradient of out[0] (NULL = 1)                          */
  float* d_cb; float* d_c; float* d_pix;   /* [N,3] bwd out                                                          */
  float* d_err;                /* [N] bwd out (every entry written)                                                  */
  float* d_sums;               /* [5] bwd out                                                                        */
  int32_t N, sums_nblk;
  float n_rays, trim_ratio;
} NudfBlendLoss;
int nudf_blend_loss_prepare(const NudfBlendLoss* args, void* stream);
int nudf_blend_loss_fwd(const NudfBlendLoss* args, void* stream);
int nudf_blend_loss_bwd(const NudfBlendLoss* args, void* stream);

/* ------------------------------------------------------------------------------------
 * ray sampling helpers (models/udf_renderer_blending.py:605-630, 352-357, 164-173, 205)
 * ---------------------------------------------------------------------------------- */
int nudf_coarse_z(const float* near, const float* far, int nf_stride, const float* t_rand, int N, int S,
                  float* z, float* sample_dist, void* stream);
/* nudf_coarse_z + the points o + d z of those samples (nudf_ray_points mode 0) in ONE launch -- the start of the
 * hierarchical sampling.  center != 0: t_rand holds the raw U[0, 1) draws and the - 0.5 of :618 is applied here
 * (one rounded subtraction, as the separate torch op).  pts [N S, 3] or NULL. */
int nudf_coarse_start(const float* near, const float* far, int nf_stride, const float* t_rand, int center, int N, int S,
                      float* z, float* sample_dist, const float* rays_o, const float* rays_d, float* pts, void* stream);
int nudf_outside_z(const float* far, int f_stride, const float* lin, int N, int n_out, int n_samples,
                   float* z_out, void* stream);
int nudf_ray_points(const float* rays_o, const float* rays_d, const float* z, const float* sample_dist, int N,
                    int S, int mode, float* pts, void* stream);

/* positional encoding value / JVP (tangent != NULL) / VJP  (models/embedder.py:15-36) */
int nudf_posenc(const float* x, int xld, int xdiv, const float* tangent, int D, int L, float in_scale, int P,
                float* dst1, int ld1, float scale1, float* dst2, int ld2, float scale2, void* stream);
int nudf_posenc_vjp(const float* x, int xld, int D, int L, float in_scale, int P, const float* src1, int ld1,
                    float scale1, const float* src2, int ld2, float scale2, float* g, void* stream);
int nudf_copy_cols(const float* src, int lds, int sdiv, float* dst, int ldd, int ncols, int P, float scale,
                   void* stream);

/* heads of the MLP chains */
int nudf_udf_grad_seed(const float* sign, const float* w_row0, const float* h, int ldh, float hscale, int P, int C,
                       float inv_scale, float* out, int ldo, void* stream);
int nudf_udf_head_bwd(const float* sign, const float* dudf, const float* dfeat, int ldf, int P, int F,
                      float scale, float* out, int ldo, void* stream);
int nudf_signed_colsum(const float* sign, const float* R, int ldr, int P, int C, float scale, float* out,
                       void* stream);
int nudf_sigmoid_head_bwd(const float* y, const float* dy, const float* dy_extra, int ldx, int nsig,
                          const float* draw, int ldr, int nraw, int P, float* out, int ldo, void* stream);

/* weight_norm packing (torch.nn.utils.weight_norm at fields.py:175-176, 433-446) and its backward */
int nudf_weightnorm_pack(const float* v, const float* g, int out, int in, const int* perm, float* W, int ldw,
                         float* Wt, int ldwt, float* inv_norm, void* stream);
int nudf_weightnorm_unpack_grad(const float* dW, int ldw, const float* v, const float* g, const float* inv_norm,
                                int out, int in, const int* perm, float* dv, float* dg, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-tensor Adam (one launch for all parameters).  Replaces the foreach kernels of
 * torch.optim.Adam.step() as the runner uses it (exp_runner_blending.py:136-139, :373-375);
 * same arithmetic, same state (exp_avg, exp_avg_sq, step).  The table is passed by value.
 * ---------------------------------------------------------------------------------- */
#define NUDF_ADAM_MAX_TENSORS 64
#define NUDF_ADAM_MAX_GROUPS 4
typedef struct NudfAdamTensor {
  float* p; const float* g; float* m; float* v;  /* param, grad, exp_avg, exp_avg_sq (device) */
  int32_t n;                                     /* elements                                   */
  int32_t group;
  float neg_step_size;                           /* -lr / (1 - beta1^t), t = this tensor's step */
  float bc2_sqrt;                                /* sqrt(1 - beta2^t)                          */
} NudfAdamTensor;
typedef struct NudfAdamGroup {
  float one_minus_beta1, beta2, one_minus_beta2, eps;
} NudfAdamGroup;
typedef struct NudfAdam {
  int32_t n_tensors; int32_t pad_;
  NudfAdamTensor t[NUDF_ADAM_MAX_TENSORS];
  int32_t block_start[NUDF_ADAM_MAX_TENSORS + 1]; /* prefix sums of ceil(n / nudf_adam_chunk())  */
  int32_t pad2_;
  NudfAdamGroup group[NUDF_ADAM_MAX_GROUPS];
  const float* dyn;                               /* NULL, or device [2 * n_tensors]: {neg_step_size, bc2_sqrt} of tensor i at
                                                     dyn[2 i], dyn[2 i + 1], overriding the by-value fields: the two numbers
                                                     that change every step (learning-rate schedule, bias corrections), so
                                                     that a captured HIP graph of the step stays valid               */
} NudfAdam;
int nudf_adam_step(const NudfAdam* args, void* stream);
int nudf_adam_chunk(void);                         /* elements one block updates                  */

/* ------------------------------------------------------------------------------------
 * Fused MLP layer chains: a tile of points stays resident in LDS across all layers of a sweep
 * (csrc/mlp_chain.hip).  Replaces, for UDFNetwork (models/fields.py:192-231), the same chains of
 * F.linear + weight_norm + Softplus and their autograd (double) backward as nudf_gemm_nn, with one
 * launch per sweep.  Weights are passed in MFMA-B fragment order (nudf_pack_frag).
 * ROW PADDING: the kernel stores whole 64-point tiles, so every buffer it writes (C1, C2, G0) or reads in
 * an epilogue (X1, X2, r1_row) must hold roundup(P, 64) rows; rows >= P are scratch.  x, v, A0 of
 * INIT_LOAD and seed_sign are read with clamped row indices and need only P rows.  P * ld < 2^31.
 * SCRATCH ROWS: rows >= P may hold ANY bit pattern on entry (NaN, Inf, huge finite values: the buffers are
 * allocated, not cleared), and no live output, no reported maximum (absmax_out, tile_amax_out) and no status
 * bit may depend on them.  A launch therefore computes the points >= P of its last tile from row P - 1
 * (clamped reads of x, v, A0 and seed_sign; r1_row is written for all padded rows by its producer) and STORES every row of every tile it runs into C1 / C2 / G0,
 * so that a later launch, which reads whole tiles of those arrays as X1 / X2 / X3, finds defined values there.
 * Rows of tiles no workgroup runs (roundup(P, tile) .. roundup(P, 64)) are never read.
 * tests/test_gpu_scratch_poison.py holds this with poisoned allocations.
 * OUTPUTS IN GENERAL, of every entry point of this header: an output buffer may hold ANY bit pattern on entry, and
 * every element of it is written on every path -- with the documented value where there is no result: +inf for a
 * depth nothing was drawn into or a distance beyond `bound`, -1 for its face, NaN for its point and barycentrics, 0
 * for a mask, a weight sum or the normal of a face without area, `fill` for a colour no view gives, the cluster's
 * mean for a minimiser that is not accepted.  No result depends on what a float buffer held before the call.
 * tests/test_gpu_blend_poison.py (blending, ray batches) and tests/test_gpu_mesh_poison.py (the mesh, meshing and
 * evaluation tools) hold this the same way, bit pattern for bit pattern.
 * ---------------------------------------------------------------------------------- */
enum {
  NUDF_CH_NONE = 0,      /* out = (acc + bias) * scale                                            */
  NUDF_CH_SOFTPLUS = 1,  /* out = softplus100(acc + bias) * scale                                 */
  NUDF_CH_MULSP = 2,     /* out = acc * softplus'(X1) * scale ; cols >= iparam > 0: C2[col-iparam] = acc*scale */
  NUDF_CH_TANGENT = 3,   /* out = acc * s * scale ; C2 = acc * X2 * 100 (1 - s),  s = softplus'(X1) */
  NUDF_CH_BWD = 4,       /* out = acc * scale * softplus'(X1) + X2                                */
  NUDF_CH_UDFHEAD = 5,   /* col 0: C2[row] = |acc + bias| * scale, C1[row] = sign                 */
  NUDF_CH_RELU = 6,      /* out = relu(acc + bias) ; C2 (optional) mirrors it                     */
  NUDF_CH_SIGMOIDN = 7,  /* cols < iparam: sigmoid -> C1 (and tile); cols >= iparam raw -> C2[col-iparam];
                            N <= iparam: C2 mirrors the sigmoid columns instead                    */
  NUDF_CH_MULMASK = 8,   /* out = (X1 > 0) ? acc * scale : 0            (ReLU backward)           */
  NUDF_CH_ADDMASK = 9,   /* out = (X1 > 0) ? (acc + X2) * scale : 0     (ReLU backward at a join) */
  NUDF_CH_RELUADD = 10,  /* out = relu(acc + bias + X2)   (skip layer whose second input part was multiplied
                            by an earlier step: NeRF's cat([input_pts, h]) is wider than the LDS tile)  */
  /* A kind that contracts NOTHING: it turns the LDS tile a finished forward sweep left behind into the initial tile of the
     input-gradient sweep, so that the two back-to-back sweeps over the same points run as ONE launch (workgroup-shared kernel,
     split modes, 32- / 64-point tiles only; nudf_mlp_chain refuses it anywhere else).  Bp, bias are unused (NULL).
     SEED: directly behind a UDFHEAD step (and the act_write = 0 steps in front of it, which leave the tile alone): the tile
       still holds the last SOFTPLUS step's activations h, the head's multiplier sign[r] is handed over on chip --
       tile[r, c] = sign[r] * r1_col[c] * scale * softplus'(h[r, c]) for c < N (xscale as in MULSP), all rows of the tile ->
       C1 [rows padded, ldc1].  The same values NUDF_CH_INIT_SEED forms from the stored arrays, bit for bit.               */
  NUDF_CH_SEED = 11
};
enum {
  NUDF_CH_INIT_LOAD = 0,   /* activation tile = A0[rows, 0:k0]                                    */
  NUDF_CH_INIT_POSENC = 1, /* activation tile = PE(x) (or its JVP with tangent v), zero-padded to k0 */
  NUDF_CH_INIT_SEED = 2    /* tile[r,c] = seed_sign[r] * seed_wrow[c] * seed_scale * softplus'(A0[r,c]) */
};
#define NUDF_CH_MAX_STEPS 20          /* forward + input gradient of a 9-layer UDF network in one launch: 19 */
typedef struct NudfChainStep {
  const float* Bp;                 /* packed weights (nudf_pack_frag) of the [K, N] operand          */
  const float* bias;               /* [N] or NULL                                                    */
  const float* X1; const float* X2;/* epilogue operands [P, ld] stored by an earlier sweep, or NULL   */
  float* C1; float* C2;            /* HBM copies of the outputs (NULL = keep in LDS only)            */
  const float* r1_row;             /* optional rank-1 term: acc += r1_row[row] * r1_col[col]         */
  const float* r1_col;
  int32_t K, N;                    /* K % 16 == 0, K <= 288, N <= 256                                */
  int32_t epi;                     /* NUDF_CH_*                                                      */
  int32_t iparam;
  int32_t ldx1, ldx2, ldc1, ldc2;
  int32_t ldr1;                    /* element stride of r1_row                                       */
  int32_t prec;                    /* MFMA operand precision: 0 = fp32 (v_mfma_f32_32x32x2_f32), 1 = fp16, 2 = bf16 (fp32
                                      accumulate; Bp then holds the 16-bit fragment layout of
                                      nudf_weightnorm_pack_multi), 3 = bf16x3: fp32 EMULATED on the bf16 matrix pipe --
                                      both operands split exactly into three bf16 parts (x = hi + mid + lo), the six
                                      products hi hi, hi mid, mid hi, hi lo, lo hi, mid mid on v_mfma_f32_32x32x16_bf16
                                      with fp32 accumulation; the dropped terms are <= 2^-23 |x| |y| per product, the size
                                      of one fp32 rounding (Bp: the three-plane layout of NudfPackFrag.dtype 3);
                                      4 = f16x2: fp32 EMULATED on the fp16 matrix pipe with THREE products -- both operands
                                      split into two fp16 parts, x = hi + 2^-11 lo (hi = fp16(x), lo = fp16((x - hi) 2^11):
                                      11 + 11 significant bits, the low part pre-scaled into fp16's normal range),
                                      acc0 += hi hi', acc1 += hi lo' + lo hi' on v_mfma_f32_32x32x16_f16, result
                                      acc0 + 2^-11 acc1 (the correction terms in their own fp32 accumulator); dropped:
                                      lo lo' <= 2^-22 |x| |y|.  For operands inside fp16's range (|x| < 65504; below
                                      6e-5 the split keeps an ABSOLUTE resolution of ~3e-11): the forward-order sweeps
                                      (encodings, activations, weight-normed weights) as they are; the backward sweeps,
                                      whose operands are adjoints of the loss, with NudfChain.tile_scale
                                      (Bp: the two-plane layout of NudfPackFrag.dtype 4)                                */
  int32_t act_write;               /* 1: the outputs become the next step's activation tile          */
  int32_t act_col0;                /* ... at tile columns [act_col0, act_col0 + N)                   */
  int32_t pe_tail_col;             /* >= 0: afterwards write PE(x)*pe_tail_scale at these tile columns ...       */
  int32_t ld_pe;
  float* pe_dst;                   /* ... and at the same columns of pe_dst [P, ld_pe] (or NULL)                */
  float pe_tail_scale;
  float scale, xscale;
  int32_t layout;                  /* NUDF_CH_BLK_* bits: which of this step's [P, ld] buffers use the BLOCKED layout */
  /* SIGMOIDN steps of the workgroup-shared kernel only -- the compositing sum of a colour head taken inside its epilogue
     (udf_renderer_blending.py:508-526: (colour * weights[..., None]).sum(dim=1)), so that the per-sample colours need not
     go to memory: row_w [rows padded to 64, zero tail] = the compositing weight of every point; row_sums [ceil(P / 32), 4]:
     row_sums[b][c] = sum over the 32 points of block b of row_w[r] * sigmoid(v[r][c]), c < min(iparam, 4) (fixed order).
     With rays of S % 32 == 0 samples the blocks of a ray are consecutive: nudf_composite_colour_finish adds them up.
     C1 / C2 may be NULL then. */
  const float* row_w;
  float* row_sums;
  /* NUDF_CH_BWD steps only (workgroup-shared kernel, split / 16-bit modes): a THIRD stored operand.  With X3 = NULL the step
     adds X2 = EX[l-1], the second-order term the tangent sweep stored (EX = (R W^T) * DA * softplus'' / softplus').  With X3 set
     the term is formed here instead, from arrays that exist anyway -- X2 = R[l] (the tangent sweep's activations, which the
     second-order weight gradient reads) and X3 = DA[l-1] (the input-gradient sweep's adjoints):
         EX = X2 * X3 * 100 (1 - s) / (s * scale),   s = softplus'(.) recovered from X1 as everywhere, 0 where s = 0
     (R = (R W^T) s scale, so R / (s scale) is the pre-activation tangent again).  The tangent sweep then neither reads DA nor
     writes EX: two of its four arrays per layer (fields.py:219-231 with create_graph=True is the reference's form of all of this). */
  const float* X3;
  int32_t ldx3;
} NudfChainStep;
/* Blocked layout of a [P, ld] buffer (P padded to 32 rows, ld % 4 == 0): element (r, c) lives at
 *   (r / 32) * 32 * ld + (c / 4) * 128 + (r % 32) * 4 + (c % 4)
 * i.e. inside every 32-row block the four-column quads are stored one after the other, 32 rows x 16 bytes each.  The
 * transposed-product chain kernel (tile_rows = 66: accumulator lane = point, registers = quads of features) then moves
 * 1 KB of CONTIGUOUS memory per wave instruction for its stored-state operands and outputs, and a [32 x 128] operand
 * tile of the weight-gradient GEMM is 16 KB contiguous.  Only that kernel and nudf_gemm_tn_grouped read the layout. */
#define NUDF_CH_BLK_X1 1
#define NUDF_CH_BLK_X2 2
#define NUDF_CH_BLK_C1 4
#define NUDF_CH_BLK_C2 8
#define NUDF_CH_BLK_PE 16           /* pe_dst */
/* config-5 mode: this step's stored-state arrays -- X1, X2, C1, the TANGENT mirror C2 and pe_dst -- hold bf16 (ld in
 * elements); SOFTPLUS / MULSP / TANGENT / BWD steps of the workgroup-shared kernels only.  Values are rounded to
 * nearest even when stored; everything on chip stays fp32.  The arrays are 4-POINT PACKED: element (row, col) of a
 * [R, ld] buffer (R a multiple of 64) sits at ((row / 4) ld + col) 4 + row % 4 -- the four consecutive points a lane of a
 * 32 x 32 accumulator tile holds for its column are one 8-byte access, and a dword is the row pair the 16-bit
 * weight-gradient GEMM contracts (NUDF_TN_A_P4 / NUDF_TN_B_P4).  The same holds for a bf16 A0 / G0 of the SEED
 * initialisation (init_state16 bits 1 / 2). */
#define NUDF_CH_STATE16 32
/* the ReLU family of the 16-bit mode (colour net): per array, because its steps also touch fp32 interface buffers (the
 * view-branch input, d VIN).  RELU: C1; MULMASK / ADDMASK: X1 and / or C1 -- bf16, 4-point packed as above. */
#define NUDF_CH_P4_X1 64
#define NUDF_CH_P4_C1 128
typedef struct NudfChain {
  int32_t P, n_steps;
  int32_t init;                    /* NUDF_CH_INIT_*                                                 */
  int32_t k0;                      /* initial tile width (multiple of 4, <= 288)                     */
  int32_t x_div;                   /* x row of point p is p / x_div (samples per ray for per-ray directions; >= 1) */
  int32_t tile_rows;               /* 0 = choose; 32 / 64 points per workgroup (shared tile); 66 = 64-point shared tile,
                                      transposed product (16-byte epilogue accesses); 128 = prefer the wave-private
                                      kernel (4 waves x 32 points);
                                      66 / 128 need fp32 steps and 16-byte aligned rows and fall back
                                      to 64 otherwise (NUDF_CH_TILE_* below; nudf_mlp_chain_plan tells what a launch gets) */
  int32_t lda0, ldg0;
  int32_t pe_L, pe_jvp;            /* positional encoding: frequencies, 1 = JVP with tangent v       */
  int32_t init_state16;            /* INIT_SEED: bit 0 = A0 holds bf16, bit 1 = G0 receives bf16, bit 2 = A0 is in the
                                      BLOCKED layout, bit 3 = G0 is (fp32, transposed-product kernel only)          */
  float pe_in_scale;
  float seed_scale, seed_xscale;
  const float* A0;                 /* INIT_LOAD source / INIT_SEED stored activation                 */
  float* G0;                       /* optional HBM copy of the initial tile [P, ldg0]                */
  const float* x;                  /* [P,3] points (positional encoding), or NULL                    */
  const float* v;                  /* [P,3] tangent (JVP), or NULL                                   */
  const float* seed_sign;          /* [P]                                                            */
  const float* seed_wrow;          /* [k0]                                                           */
  unsigned long long* dbg;         /* NULL, or [blocks*4 waves][64] timeline: hw_id, t0, per step (K loop end,
                                      after barrier 1, epilogue end, after barrier 2) in s_memtime ticks */
  float* absmax_out;               /* NULL, or ONE device float (zeroed by the caller; split modes of the workgroup-shared kernel):
                                      the launch raises it (atomic max) to the largest |value| it puts into the stored arrays a
                                      weight-gradient GEMM will read -- the initial tile (INIT_LOAD values; for the JVP encoding the
                                      bound 2^(L-1) |v| in_scale), every C1 / pe-free output of its MULSP / BWD / MULMASK / ADDMASK /
                                      NONE steps, and the rank-1 operand r1_row.  It is what scales that side of an f16x2 GEMM
                                      (NudfGemmTNGroup.amax_a / amax_b).                                                      */
  /* Per-tile scaling of a LINEAR sweep (split modes of the workgroup-shared kernel; what lets the backward sweeps -- whose
     operands are adjoints of the LOSS, 1e-5 ... 1e-12 -- contract as f16x2, prec 4).  The tangent, adjoint and ReLU-backward
     sweeps map each point's seeds linearly to that point's outputs, so a tile of points may run multiplied by any power of two:
     tile_scale = 1 makes the kernel take m = the largest |seed| of its tile -- the initial tile (INIT_LOAD values; for the JVP
     encoding the bound 2^(L-1) |v| in_scale), the rank-1 operands of its steps, tile_amax_in -- and sigma = 2^(-6 - floor(log2 m));
     the activation tile then holds sigma times the sweep's values (largest seed in [2^-6, 2^-5): 2^21 of growth below fp16's
     largest number; elements down to 2^-8 of the seed keep all 22 bits of the split, smaller ones 2^-30 of the seed absolutely),
     operands that enter from memory (r1_row, X2 of BWD / ADDMASK) are multiplied by sigma and everything that goes to memory (G0,
     C1, C2, pe_dst) by 1 / sigma -- powers of two, exact: memory holds what it held without the option.  Requires a
     linear chain: INIT_LOAD or the JVP encoding, steps NONE / MULSP / TANGENT / BWD / MULMASK / ADDMASK without bias.
     A tile of zero seeds runs with sigma = 1.
     tile_amax_in: NULL or [rows padded to 64 / 32] floats, per 32 points a bound of what ENTERS later in the sweep (X2), merged
     into m; tile_amax_out: NULL or the same shape, receives per 32 points the largest |value| this launch stored for them (what
     absmax_out reduces over the whole launch) -- the tangent sweep's is the adjoint sweep's tile_amax_in. */
  const float* tile_amax_in;
  float* tile_amax_out;
  int32_t tile_scale;
  int32_t reserved0;
  NudfChainStep step[NUDF_CH_MAX_STEPS];
} NudfChain;
#define NUDF_CH_TILE_TQ 66            /* NudfChain.tile_rows: the transposed-product shared tile (mlp_chain_tq_kernel)  */
#define NUDF_CH_TILE_ROWS 128         /* ... the wave-private kernel (mlp_chain_rows_kernel)                            */
#if defined(__cplusplus)
static_assert(sizeof(NudfChain) <= 4096, "NudfChain travels by value: the kernel-argument segment holds 4 KB");
#endif
int nudf_mlp_chain(const NudfChain* args, void* stream);
/* which kernel nudf_mlp_chain gives this descriptor (host code only: the launcher's own check and selection, nothing the
 * descriptor points to is read, nothing is launched).  name (capacity bytes) receives the instantiation as spelled in the
 * source -- "mlp_chain_kernel<64, 2>", "mlp_chain_tq_kernel<1, 3, true>", ... -- and out[0..3] = {grid.x, block.x, 0, 0}.
 * Returns what nudf_mlp_chain would return before launching: 0, or the error of a refused descriptor (text in
 * nudf_last_error, empty name, zero grid).  An empty launch (P <= 0 or no steps) gives 0, an empty name and a zero grid.
 * The choice depends on the process-wide settings NUDF_CHAIN_ROWS / _QUAD / _T16 / _WIN2. */
int nudf_mlp_chain_plan(const NudfChain* args, char* name, int capacity, int32_t* out);
/* 16-bit mode (prec 1 / 2), 64-point tiles: chains whose steps ALL contract in the same 16-bit type run on the 16-bit-tile
 * kernel -- the LDS activation tile holds that type (the MFMA operand itself: one ds_read_b128 per 32-row tile and k step, no
 * conversion in the K loop, 37 KB per workgroup = three workgroups per CU), the epilogue rounds the new activations once on
 * their way into the tile.  Bit-identical to the fp32-tile kernel (same values rounded to the same type).  0 switches it off
 * (A/B, tests; env NUDF_CHAIN_T16); returns the old setting. */
int nudf_set_chain_t16(int on);
/* out[((g*NT + T)*64 + lane)*4 + j] = B[8g + 4(lane>>5) + j][32T + (lane&31)], zero outside K x N;
 * out holds roundup(K,16)/8 * roundup(N,32)/32 * 256 floats */
int nudf_pack_frag(const float* B, int ldb, int K, int N, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-layer weight packing in ONE launch (table by value): weight_norm (W = g v/|v|), the two GEMM layouts
 * and the MFMA-fragment copies the fused chains read (nudf_pack_frag layout), for up to 16 layers; and the
 * matching multi-layer backward of the packing.  Same arithmetic as nudf_weightnorm_pack / _unpack_grad
 * (torch.nn.utils.weight_norm at fields.py:175-176, 433-446).
 * ---------------------------------------------------------------------------------- */
#define NUDF_PACK_MAX_LAYERS 16
#define NUDF_PACK_MAX_FRAGS 4
typedef struct NudfPackFrag {
  float* dst;                      /* fragment-ordered [K, N] operand (zero-initialised by the caller once)     */
  int32_t transpose;               /* 1: B[k][n] = W[o0 + n][i0 + k] (W^T, forward sweeps); 0: B[k][n] = W[o0 + k][i0 + n] */
  int32_t o0, i0;                  /* offsets into the packed [out, in] matrix                                  */
  int32_t K, N;
  int32_t dtype;                   /* 0: fp32 fragments (nudf_pack_frag layout); 1 / 2: fp16 / bf16 fragments for
                                      v_mfma_f32_32x32x16_*: dst16[((g*NT + T)*64 + lane)*8 + j] =
                                      B[16g + 8(lane>>5) + j][32T + (lane&31)], round-to-nearest-even;
                                      3: bf16x3 split, three planes hi / mid / lo of that layout stored back to back per
                                      (g, T): dst16[(((g*NT + T)*3 + plane)*64 + lane)*8 + j]  (3x the 16-bit size);
                                      4: f16x2 split, two fp16 planes hi = fp16(w), lo = fp16((w - hi) 2^11):
                                      dst16[(((g*NT + T)*2 + plane)*64 + lane)*8 + j]  (2x the 16-bit size)            */
} NudfPackFrag;
typedef struct NudfPackLayer {
  const float* v; const float* g;  /* weight_v [out,in], weight_g [out] (NULL: plain Linear)                    */
  const int32_t* perm;             /* input-column permutation or NULL                                          */
  float* W; float* Wt;             /* [out_pad, ldw], [in_pad, ldwt] (either may be NULL)                       */
  float* inv_norm;                 /* [out] 1/|v_row| (kept for the backward) or NULL                           */
  int32_t out, in, ldw, ldwt;
  int32_t nfrag, row_start;        /* row_start: prefix sum of `out` over the preceding layers                  */
  NudfPackFrag frag[NUDF_PACK_MAX_FRAGS];
} NudfPackLayer;
typedef struct NudfPackMulti {
  int32_t n_layers, total_rows;
  NudfPackLayer layer[NUDF_PACK_MAX_LAYERS];
} NudfPackMulti;
int nudf_weightnorm_pack_multi(const NudfPackMulti* args, void* stream);

typedef struct NudfUnpackLayer {
  const float* dW;                 /* [out_pad, ldw] packed weight gradient                                     */
  const float* v; const float* g; const float* inv_norm;
  const int32_t* perm;
  float* dv; float* dg;            /* [out,in], [out] (dg NULL for a plain Linear)                              */
  const float* db_in; float* db_out; /* optional [out] copy of the bias gradient out of the flat packed buffer  */
  int32_t out, in, ldw, row_start;
} NudfUnpackLayer;
typedef struct NudfUnpackMulti {
  int32_t n_layers, total_rows;
  NudfUnpackLayer layer[NUDF_PACK_MAX_LAYERS];
} NudfUnpackMulti;
int nudf_weightnorm_unpack_grad_multi(const NudfUnpackMulti* args, void* stream);

/* ------------------------------------------------------------------------------------
 * The three learnable scalars of the renderer in one launch (instead of ~15 one-element torch kernels):
 *   inv_s = exp(10 variance).clip(1e-6, 1e6)                      fields.py:654-655, udf_renderer_blending.py:373
 *   beta  = exp(10 beta).clip(0, beta_hi).clip(1e-6, 1e6)          fields.py:674-675, :376   (beta_hi = 1/beta_min)
 *   gamma = exp(10 gamma).clip(1e-6, 1e6)                          fields.py:677-678, :377
 * scal[3] = {inv_s, beta, gamma}; recip[2] = {1/inv_s, 1/beta} (the 'variance' / 'beta' entries of render()).
 * bwd: d_param[3] = d_scal * d scal / d param (torch.clip passes the gradient on the closed interval).
 * ---------------------------------------------------------------------------------- */
int nudf_scalars_fwd(const float* variance, const float* beta, const float* gamma, float beta_hi, float* scal,
                     float* recip, void* stream);
int nudf_scalars_bwd(const float* variance, const float* beta, const float* gamma, float beta_hi, const float* d_scal,
                     float* d_param, void* stream);

/* sum_i |pred_i - gt_i| (the numerator of ColorPixelLoss, loss/loss.py:37-43) and its backward
 * d_pred_i = d_out * sign(pred_i - gt_i).  out[0] = sum (one workgroup: these are [N,3] tensors). */
int nudf_l1_sum_fwd(const float* pred, const float* gt, int n, float* out, void* stream);
int nudf_l1_sum_bwd(const float* pred, const float* gt, int n, const float* d_out, float* d_pred, void* stream);

/* batch-global regularisers from the composite kernel's partial sums (udf_renderer_blending.py:531-536, 553):
 *   err[0] = sums[0] / (sums[1] + 1e-5), err[1] = sums[2] / (sums[3] + 1e-5), err[2] = sums[4] / n_rays
 * bwd: d_sums[5] (entries 1 and 3, the mask counts, included for completeness). */
int nudf_sums_errors_fwd(const float* sums, float n_rays, float* err, void* stream);
int nudf_sums_errors_bwd(const float* sums, float n_rays, const float* d_err, float* d_sums, void* stream);

/* Loss weights in device memory.  The runner's schedules move the colour weights and the regulariser weights from
 * iteration to iteration (adjust_color_loss_weights, exp_runner_blending.py:230-251; regularization_weights_schedule,
 * :199-211), and a step captured in a HIP graph replays the kernel ARGUMENTS of its capture: every loss entry point
 * below therefore takes `w_dev`, NULL or a device vector of NUDF_LW_COUNT floats laid out by the NUDF_LW_* indices,
 * whose entries override the by-value weights of the same call. */
enum { NUDF_LW_COLOR_BASE = 0, NUDF_LW_COLOR = 1, NUDF_LW_COLOR_PIXEL = 2, NUDF_LW_COLOR_PATCH = 3, NUDF_LW_IGR = 4,
       NUDF_LW_IGR_NS = 5, NUDF_LW_SPARSE = 6, NUDF_LW_MASK = 7,
       NUDF_LW_COLOR_SUM = 8,      /* color_base + color + color_pixel formed by the host in double (the host-side mirror's
                                      torch expressions divide by it; the kernels form the sum themselves in fp32) */
       NUDF_LW_COUNT = 16 };

/* ColorLoss in one launch when only the two L1 terms are active (loss/loss.py:105-133 with color_pixel = None,
 * patch_colors = None):  den = mask ? sum(mask) + 1e-4 : n ;  Lb = sum|cb - gt| / den ;  Lc = sum|c - gt| / den ;
 * out[3] = {(Lb w_b + Lc w_c) / (w_b + w_c + w_px), Lb, Lc}.
 * bwd: d_cb / d_c from the upstream gradients d_out[3] (any of which may be zero). */
int nudf_color_loss_fwd(const float* cb, const float* c, const float* gt, int n, const float* mask, int n_mask,
                        float w_b, float w_c, float w_px, const float* w_dev, float* out, float* den_out, void* stream);
int nudf_color_loss_bwd(const float* cb, const float* c, const float* gt, int n, const float* den, float w_b, float w_c,
                        float w_px, const float* w_dev, const float* d_out, float* d_cb, float* d_c, void* stream);
/* the same loss split at the ray-sharding exchange step (one process per GPU): local sums[3] = {sum|cb - gt|,
 * sum|c - gt|, sum(mask) or n} -> the caller all-reduces them (RCCL) -> finish forms out[3] / den exactly as above;
 * nudf_color_loss_bwd then runs on the local rays with the GLOBAL den. */
int nudf_color_loss_sums(const float* cb, const float* c, const float* gt, int n, const float* mask, int n_mask,
                         float* sums, void* stream);
int nudf_color_loss_finish(const float* sums, int has_mask, float w_b, float w_c, float w_px, const float* w_dev,
                           float* out, float* den_out, void* stream);

/* The whole loss assembly of a train step when only the two L1 colour terms and the three regularisers are active
 * (exp_runner_blending.py:330-371; loss/loss.py:105-133; udf_renderer_blending.py:531-536, 553): nudf_color_loss_fwd +
 * nudf_sums_errors_fwd + total = ((cl + gens w_igr_ns) + sparse w_sparse) + ge w_igr in one launch, each product / sum
 * of the last line rounded on its own like the runner's scalar torch ops.  out[8] = {total, cl, Lb, Lc, ge, gens,
 * sparse, 0}; den_out[1].  bwd: upstream d_total (device scalar, NULL = 1) and optionally d_extra[8] for the other
 * outputs (indexed like out[], NULL = none) -> d_cb / d_c [n] and d_sums[5].
 * sums_ws != NULL: the composite kernel left its per-block partial sums [sums_nblk, 5] there (NudfComposite.defer_sums);
 * this launch reduces them first (nudf_partial_sums' order) and WRITES the five sums to `sums` as well. */
int nudf_step_loss_fwd(const float* cb, const float* c, const float* gt, int n, const float* mask, int n_mask,
                       float* sums, float n_rays, float w_b, float w_c, float w_px, float w_igr, float w_igr_ns,
                       float w_sparse, const float* w_dev, float* out, float* den_out, const float* sums_ws,
                       int sums_nblk, void* stream);
int nudf_step_loss_bwd(const float* cb, const float* c, const float* gt, int n, const float* den, const float* sums,
                       float n_rays, float w_b, float w_c, float w_px, float w_igr, float w_igr_ns, float w_sparse,
                       const float* w_dev, const float* d_total, const float* d_extra, float* d_cb, float* d_c, float* d_sums,
                       void* stream);
/* out4 [P_pad, 4] (16-byte aligned): column 0 = sign[r] * d[r] * scale (d NULL: sign[r] * scale) for r < P, everything
 * else zero: the 4-wide column-0 operand of the UDF head's adjoint and second-order weight gradient (fields.py:184-231) */
/* out4_sign (NULL or like out4): column 0 = sign[r] * scale, written by the same launch */
int nudf_col0_seed4(const float* sign, const float* d, float scale, int P, int P_pad, float* out4, float* out4_sign,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * GPU-resident ray / patch batch generation: Dataset.gen_random_rays_patches_at (dataset/dataset.py:228-294) and
 * Dataset.near_far_from_sphere (:329-335) in one call.  The pixel coordinates are drawn by the caller
 * (torch.randint keeps the reference's RNG semantics).
 * ---------------------------------------------------------------------------------- */
typedef struct NudfRayBatch {
  const float* image;              /* [H, W, 3] colours of the reference view (images[img_idx])                 */
  const float* mask;               /* [H, W, 3]                                                                  */
  const float* intrinsics_inv;     /* [4, 4] row-major                                                           */
  const float* pose;               /* [4, 4] row-major camera-to-world                                           */
  const int64_t* pixels_x; const int64_t* pixels_y;   /* [N]                                                     */
  int32_t N, H, W, h_patch_size;
  float* rays;                     /* [N, 10] = rays_o 3 | rays_v 3 | colour 3 | mask 1                          */
  float* ndc_uv;                   /* [N, 2] or NULL                                                             */
  float* xyz_cam;                  /* [N, 3] K^-1 (x, y, 1) or NULL                                              */
  float* near; float* far;         /* [N] each, or both NULL                                                     */
  float* patch_color;              /* [N, (2h+1)^2, 3] or NULL (crop_patch = False)                              */
  uint8_t* patch_mask;             /* [N] or NULL                                                                */
} NudfRayBatch;
int nudf_gen_ray_batch(const NudfRayBatch* args, void* stream);

/* ------------------------------------------------------------------------------------
 * MeshUDF open-surface extraction from a dense UDF grid (MeshUDF, Guillard et al. 2022): replaces the Cython mesher
 * custom_mc/_marching_cubes_lewiner_cy.pyx udf_mc_lewiner (:1115-) that extract_mesh.py get_mesh_udf_fast (:169-354)
 * calls from Runner.extract_udf_mesh (exp_runner_blending.py:763-800).  Pseudo-signs are chosen per cell with no
 * propagation between cells (the reference's serial sign-propagation queue is not reproduced): corner r = the corner of
 * largest U (lowest index on ties) is `+`, corner c is `+` iff dot(G_r, G_c) >= 0 in float64.  A cell is active when the
 * fp32 mean of its 8 corner values is < mean_thr and their max is <= max_thr (pyx :1157-1158).  The 256-case table is
 * generated by neuraludf_amd/mc_tables.py (csrc/mc_tables.inc).  Three launches; the scans and compactions between them
 * are the caller's (deterministic integer prefix sums).  Grid: N^3 points x-major, lin(i, j, k) = (i N + j) N + k;
 * cell (i, j, k) < N - 1 has lowest corner lin(i, j, k) and compact index (i (N-1) + j) (N-1) + k; edge id
 * 3 lin(lower end) + axis.  3 <= N <= 1024.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfMeshUDF {
  const float* U;            /* [N, N, N] UDF values                                                                 */
  const float* G;            /* [N, N, N, 3] UDF gradients (read at the corners of active cells only)                */
  const float* axes;         /* [3, N] grid coordinate of each index, per axis                                      */
  uint8_t* cell_case;        /* [(N-1)^3] case index (bit c set: corner c is `-`), 0 for inactive cells (classify)    */
  uint8_t* cell_ntri;        /* [(N-1)^3] triangles of the cell (classify)                                           */
  uint8_t* edge_flag;        /* [3 N^3] zeroed by the caller; classify stores 1 at every sign-change edge of an active
                                cell that emits triangles                                                            */
  const int64_t* cells;      /* [n_cells] compact indices of the cells with triangles, ascending (emit)               */
  const int64_t* face_off;   /* [n_cells] exclusive prefix sum of their triangle counts (emit)                       */
  const int64_t* edge_scan;  /* [3 N^3] inclusive prefix sum of edge_flag: vertex of edge e = edge_scan[e] - 1 (emit)  */
  int64_t* faces;            /* [F, 3] vertex indices (emit)                                                         */
  const int64_t* edges;      /* [n_edges] ids of the flagged edges, ascending (vertices)                             */
  float* verts;              /* [n_edges, 3] vertex positions at t = U_a / (U_a + U_b) from the lower end a (vertices) */
  int64_t n_cells;
  int64_t n_edges;
  int64_t n_faces;           /* F: emit refuses a face_off that would write past faces[F]                           */
  int32_t N;
  float mean_thr;            /* 1.05 h, h = the largest grid spacing                                                */
  float max_thr;             /* 1.74 h                                                                               */
  int32_t pad_;
} NudfMeshUDF;
int nudf_meshudf_classify(const NudfMeshUDF* args, void* stream);   /* one thread per cell   */
int nudf_meshudf_emit(const NudfMeshUDF* args, void* stream);       /* one thread per cell with triangles */
int nudf_meshudf_vertices(const NudfMeshUDF* args, void* stream);   /* one thread per flagged edge */

/* ------------------------------------------------------------------------------------
 * Sparse MeshUDF extraction: the mesher above over the B^3-cell blocks near the surface only (neuraludf_amd/meshing.py
 * udf_sparse_grid, udf_marching_cubes_sparse).  The grid is the dense one (N nodes per axis, M = N - 1 cells).  Blocks:
 * nb = ceil(M / B) per axis, B in {4, 8}; block (bi, bj, bk), linear id (bi nb + bj) nb + bk, covers the cells
 * [b B, min((b + 1) B, M)) per axis.  Selection rule (the caller's, part of the contract): with the per-axis spacings
 * h_a = (bound_max[a] - bound_min[a]) / (N - 1), h = max_a h_a, the block half-diagonal r = sqrt(sum_a (B h_a)^2) / 2 and
 * thr = 1.74 h + lipschitz r (float64, rounded up to fp32), a block is selected iff the minimum of the UDF (clamped at 0)
 * at its eight coarse corners -- the nodes min(b B, N - 1) and min((b + 1) B, N - 1) per axis -- is <= thr; a NaN corner
 * never selects.  Every point of a block lies within r of a corner, and an active cell has all corners <= 1.74 h, so
 * with |grad U| <= lipschitz no active cell lies outside a selected block.
 * Storage: the K selected blocks ascending; brick s holds the (B + 1)^3 nodes (b B + a) of its block, local index
 * (ax (B + 1) + ay) (B + 1) + az; nodes past the grid's end in ragged blocks are padding and are never read.  Every
 * copy of a shared node must hold the same bits (the caller queries each node once).
 * Ordering contract, identical to the dense mesher's: vertices ascending by global edge id 3 lin(lower end) + axis,
 * lin(i, j, k) = (i N + j) N + k; faces by ascending global cell index (i M + j) M + k, then table order.  The caller
 * sorts the cells with triangles and the unique edge keys (deterministic integer sorts over active cells and edges
 * only); no output position depends on timing.  3 <= N <= 4096.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfMeshUDFSparse {
  const float* U;             /* [K, (B+1)^3] brick UDF values                                                       */
  const float* G;             /* [K, (B+1)^3, 3] brick UDF gradients (read at the corners of active cells only)       */
  const float* axes;          /* [3, N] grid coordinate of each index, per axis                                      */
  const int64_t* blocks;      /* [K] linear ids of the selected blocks, ascending                                    */
  const int32_t* block_slot;  /* [nb^3] brick of a block, -1: not selected                                           */
  uint8_t* cell_case;         /* [K, B^3] case index per brick cell, 0 for inactive cells and cells past the grid (classify) */
  uint8_t* cell_ntri;         /* [K, B^3] triangles of the cell (classify)                                           */
  const int64_t* cells;       /* [n_cells] global indices (i M + j) M + k of the cells with triangles, ascending       */
  const int64_t* face_off;    /* [n_cells] exclusive prefix sum of their triangle counts (emit)                      */
  int64_t* edge_keys;         /* [n_cells, 12] global id of every sign-change edge of the cell, INT64_MAX for the other
                                 edges (edges)                                                                       */
  const int64_t* edges;       /* [n_edges] the unique edge ids, ascending (emit: vertex of an edge = its position;
                                 vertices)                                                                           */
  int64_t* faces;             /* [F, 3] vertex indices (emit)                                                        */
  float* verts;               /* [n_edges, 3] vertex positions at t = U_a / (U_a + U_b) from the lower end a (vertices) */
  int64_t n_blocks;           /* K                                                                                   */
  int64_t n_cells;
  int64_t n_edges;
  int64_t n_faces;            /* F: emit refuses a face_off that would write past faces[F]                           */
  int32_t N;
  int32_t B;                  /* 4 or 8                                                                              */
  int32_t nb;                 /* ceil((N - 1) / B)                                                                   */
  float mean_thr;             /* 1.05 h, h = the largest grid spacing                                                */
  float max_thr;              /* 1.74 h                                                                               */
  int32_t pad_;
} NudfMeshUDFSparse;
int nudf_meshudf_sparse_classify(const NudfMeshUDFSparse* args, void* stream);  /* one workgroup per brick, its U in LDS */
int nudf_meshudf_sparse_edges(const NudfMeshUDFSparse* args, void* stream);     /* one thread per cell with triangles */
int nudf_meshudf_sparse_emit(const NudfMeshUDFSparse* args, void* stream);      /* one thread per cell with triangles */
int nudf_meshudf_sparse_vertices(const NudfMeshUDFSparse* args, void* stream);  /* one thread per unique edge */

/* ------------------------------------------------------------------------------------
 * Level-set marching cubes of a dense scalar grid: the surface {F = level} of a signed or unsigned field
 * (neuraludf_amd/meshing.py iso_marching_cubes).  Replaces the PyMCubes call of extract_geometry
 * (models/udf_renderer_blending.py:52-63, reached from Runner.validate_mesh, exp_runner_blending.py:746-761) and meshes
 * the zero set of SDF networks, which the MeshUDF mesher above is not meant for.  Sign rule: corner c of a cell is `-`
 * iff F_c < level (fp32 compare); a cell with any non-finite corner (NaN, +-inf) has case 0 and emits nothing.  The
 * 256-case table is the generated one (csrc/mc_tables.inc): the triangulation of ambiguous cases, the winding (normals
 * point to the `+` side, F >= level) and all orders are this library's, only the vertex set is that of any marching
 * cubes -- one vertex per sign-change edge at t = (level - F_a) / (F_b - F_a) from the lower end a, every operation an
 * explicit fp32 rounding, t clamped to [0, 1] and 0.5 where it is NaN.  Grid, cell and edge numbering, the three
 * launches and the ordering contract are NudfMeshUDF's: vertices ascending by edge id 3 lin(lower end) + axis, faces by
 * ascending cell index, then table order; the scans and compactions between the launches are the caller's
 * (deterministic integer prefix sums).  3 <= N <= 1024.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfIsoSurface {
  const float* F;            /* [N, N, N] field values                                                               */
  const float* axes;         /* [3, N] grid coordinate of each index, per axis                                      */
  uint8_t* cell_case;        /* [(N-1)^3] case index (bit c set: F_c < level), 0 for cells with a non-finite corner (classify) */
  uint8_t* cell_ntri;        /* [(N-1)^3] triangles of the cell (classify)                                           */
  uint8_t* edge_flag;        /* [3 N^3] zeroed by the caller; classify stores 1 at every sign-change edge of a cell that
                                emits triangles                                                                      */
  const int64_t* cells;      /* [n_cells] compact indices of the cells with triangles, ascending (emit)               */
  const int64_t* face_off;   /* [n_cells] exclusive prefix sum of their triangle counts (emit)                       */
  const int64_t* edge_scan;  /* [3 N^3] inclusive prefix sum of edge_flag: vertex of edge e = edge_scan[e] - 1 (emit)  */
  int64_t* faces;            /* [F, 3] vertex indices (emit)                                                         */
  const int64_t* edges;      /* [n_edges] ids of the flagged edges, ascending (vertices)                             */
  float* verts;              /* [n_edges, 3] vertex positions (vertices)                                             */
  int64_t n_cells;
  int64_t n_edges;
  int64_t n_faces;           /* F: emit refuses a face_off that would write past faces[F]                           */
  int32_t N;
  float level;
} NudfIsoSurface;
int nudf_isosurface_classify(const NudfIsoSurface* args, void* stream);  /* one thread per cell   */
int nudf_isosurface_emit(const NudfIsoSurface* args, void* stream);      /* one thread per cell with triangles */
int nudf_isosurface_vertices(const NudfIsoSurface* args, void* stream);  /* one thread per flagged edge */

/* ------------------------------------------------------------------------------------
 * Sparse level-set marching cubes: the mesher above over the B^3-cell blocks that can hold a cut cell only
 * (neuraludf_amd/meshing.py iso_sparse_grid, iso_marching_cubes_sparse).  Blocks, bricks, padding and the ordering
 * contract are NudfMeshUDFSparse's, without gradients.  Selection rule (the caller's, part of the contract): with
 * h_a = (bound_max[a] - bound_min[a]) / (N - 1), the block half-diagonal r = sqrt(sum_a (B h_a)^2) / 2, and cmin / cmax
 * the minimum / maximum of the field at the block's eight coarse corners, a block is selected iff
 * cmin - lipschitz r <= level and cmax + lipschitz r >= level (level: the fp32 value the kernels compare with; the bounds
 * level + lipschitz r and level - lipschitz r are evaluated in float64 and rounded outward to fp32); a NaN corner never
 * selects.  Every node of a block lies within r of a corner and a cut cell has a node below the level and one at or above
 * it, so with |grad F| <= lipschitz no cut cell lies outside a selected block.  The output is the mesh the dense mesher
 * gives on the same values, in the same order.  3 <= N <= 4096.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfIsoSurfaceSparse {
  const float* F;             /* [K, (B+1)^3] brick field values                                                     */
  const float* axes;          /* [3, N] grid coordinate of each index, per axis                                      */
  const int64_t* blocks;      /* [K] linear ids of the selected blocks, ascending                                    */
  const int32_t* block_slot;  /* [nb^3] brick of a block, -1: not selected                                           */
  uint8_t* cell_case;         /* [K, B^3] case index per brick cell, 0 for cells with a non-finite corner and cells past
                                 the grid (classify)                                                                 */
  uint8_t* cell_ntri;         /* [K, B^3] triangles of the cell (classify)                                           */
  const int64_t* cells;       /* [n_cells] global indices (i M + j) M + k of the cells with triangles, ascending       */
  const int64_t* face_off;    /* [n_cells] exclusive prefix sum of their triangle counts (emit)                      */
  int64_t* edge_keys;         /* [n_cells, 12] global id of every sign-change edge of the cell, INT64_MAX for the other
                                 edges (edges)                                                                       */
  const int64_t* edges;       /* [n_edges] the unique edge ids, ascending (emit: vertex of an edge = its position;
                                 vertices)                                                                           */
  int64_t* faces;             /* [F, 3] vertex indices (emit)                                                        */
  float* verts;               /* [n_edges, 3] vertex positions (vertices)                                            */
  int64_t n_blocks;           /* K                                                                                   */
  int64_t n_cells;
  int64_t n_edges;
  int64_t n_faces;            /* F: emit refuses a face_off that would write past faces[F]                           */
  int32_t N;
  int32_t B;                  /* 4 or 8                                                                              */
  int32_t nb;                 /* ceil((N - 1) / B)                                                                   */
  float level;
} NudfIsoSurfaceSparse;
int nudf_isosurface_sparse_classify(const NudfIsoSurfaceSparse* args, void* stream);  /* one workgroup per brick, its F in LDS */
int nudf_isosurface_sparse_edges(const NudfIsoSurfaceSparse* args, void* stream);     /* one thread per cell with triangles */
int nudf_isosurface_sparse_emit(const NudfIsoSurfaceSparse* args, void* stream);      /* one thread per cell with triangles */
int nudf_isosurface_sparse_vertices(const NudfIsoSurfaceSparse* args, void* stream);  /* one thread per unique edge */

/* ------------------------------------------------------------------------------------
 * Point-cloud geometry of the Chamfer evaluation (neuraludf_amd/evaluation.py): replaces the mesh sampling, the radius
 * down-sampling and the two sklearn KD-tree nearest-neighbour sweeps of evaluation/eval_dtu_python.py (:205-370) and
 * eval_deepfashion_python.py (:62-215).  All coordinates are float64 and every expression follows the reference's
 * (numpy's / sklearn's) operation order without contraction, so the results equal a numpy restatement bit for bit.
 * One struct; each entry point reads the fields its comment names.
 *   tri_count   one thread per face: tri_n[f] = points of face f (0 for faces the reference drops, cap + 1 when more
 *               than cap);
 *   tri_emit    one thread per face: its points at out[out_base + tri_off[f] ...];
 *   keys        one thread per point: keys[s] = packed cell of pts[s] (21 bits per axis, clamped into the grid);
 *   cells       one thread per occupied cell r: inserts cell_key[r] -> r into the hash (hash_key zeroed to -1 by the
 *               caller; hash_cap a power of two >= 2 n_cells);
 *   thin_round  one thread per point (pts, keys, rank, state in cell-sorted order): state 0 undecided, 1 keep, 2 drop;
 *               adds 1 to *undecided for every point left undecided;
 *   nearest     one thread per query: dist / idx [query_idx[t]] = the float64 distance to the nearest of pts and its
 *               rank (lowest rank on ties), +inf / -1 when that is beyond bound.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfPointCloud {
  const double* verts;       /* [n_verts, 3] mesh vertices (tri_*)                                                   */
  const int64_t* faces;      /* [n_faces, 3] (tri_*)                                                                 */
  int64_t* tri_n;            /* [n_faces] points per face (written by tri_count, read by tri_emit)                   */
  const int64_t* tri_off;    /* [n_faces] exclusive prefix sum of tri_n (tri_emit)                                   */
  double* out;               /* [n_out, 3] sampled points (tri_emit)                                                 */
  int64_t n_verts;
  int64_t n_faces;
  int64_t n_out;
  int64_t out_base;          /* row of the first triangle point (the vertices come first)                            */
  int64_t cap;               /* largest point count the caller accepts                                              */
  double density;            /* the reference's downsample_density                                                   */
  const double* pts;         /* [n, 3] indexed points, cell-sorted for cells / thin_round / nearest                  */
  int64_t n;
  double origin[3];          /* lowest corner of the grid                                                            */
  double cell;               /* cell edge                                                                            */
  int32_t grid[3];           /* cells per axis, <= 2^21                                                              */
  int32_t pad_;
  int64_t* keys;             /* [n] packed cells (keys: written; thin_round: read)                                    */
  const int64_t* cell_key;   /* [n_cells] the occupied cells, ascending                                              */
  const int64_t* cell_start; /* [n_cells] first sorted point of each                                                 */
  const int64_t* cell_count; /* [n_cells]                                                                            */
  int64_t n_cells;
  int64_t* hash_key;         /* [hash_cap] -1 = empty                                                                */
  int64_t* hash_row;         /* [hash_cap]                                                                           */
  int64_t hash_cap;
  const int64_t* rank;       /* [n] position of each sorted point in the caller's order (shuffle rank / index)       */
  uint8_t* state;            /* [n] thin_round                                                                       */
  int32_t* undecided;        /* one counter, zeroed by the caller before each round                                  */
  double r2;                 /* thin_round: radius * radius                                                          */
  const double* query;       /* [n_query, 3] (nearest; cell-sorted for coherence)                                    */
  const int64_t* query_idx;  /* [n_query] output row of each query                                                   */
  int64_t n_query;
  double bound;              /* distances beyond it are reported as +inf / -1                                        */
  double box_bound2;         /* a query whose squared distance to [box_lo, box_hi] exceeds it is beyond bound        */
  double box_lo[3];
  double box_hi[3];
  double* dist;              /* [n_query] float64 sqrt(((dx dx) + (dy dy)) + (dz dz))                               */
  int64_t* idx;              /* [n_query] nearest: the rank of the nearest point; closest: the face                  */
  /* point-to-mesh distance (ABI 111, appended): tribin_count / tribin_emit / closest                                 */
  int64_t* md_ref_n;         /* [n_faces] cells touched by each face's box (written by tribin_count, read by emit)   */
  const int64_t* md_ref_off; /* [n_faces] exclusive prefix sum of md_ref_n (tribin_emit)                             */
  int64_t* md_ref_key;       /* [md_n_refs] packed cell of each (cell, face) reference (tribin_emit)                 */
  int64_t* md_ref_face;      /* [md_n_refs] its face (tribin_emit)                                                   */
  int64_t md_n_refs;
  const int64_t* md_cell_face; /* [md_n_refs] the faces by cell: md_ref_face sorted by md_ref_key, stable (closest) */
  double* md_point;          /* [n_query, 3] the closest point (closest)                                             */
  double* md_bary;           /* [n_query, 3] its barycentric weights at the face's corner order (closest, raycast)   */
  /* rays against the mesh (appended, the version stays 111: see nudf_pc_raycast below): raycast                      */
  const double* md_ray_o;    /* [n_query, 3] ray origins (sorted by the cell of entry for coherence)                 */
  const double* md_ray_d;    /* [n_query, 3] ray directions, need not be unit: t is in units of the direction       */
  double md_t_min;           /* the window t_min <= t <= t_max of every ray ...                                      */
  double md_t_max;
  const double* md_ray_window; /* ... or NULL, or [n_query, 2] a (t_min, t_max) per ray, which then replaces the two */
  int32_t md_mode;           /* 0 first hit, 1 any hit, 2 count of the faces crossed                                 */
  int32_t md_pad_;
  int64_t* md_count;         /* [n_query] any: 0 / 1; count: the faces crossed in the window                         */
} NudfPointCloud;
int nudf_pc_tri_count(const NudfPointCloud* args, void* stream);   /* one thread per face  */
int nudf_pc_tri_emit(const NudfPointCloud* args, void* stream);    /* one thread per face  */
int nudf_pc_keys(const NudfPointCloud* args, void* stream);        /* one thread per point */
int nudf_pc_cells(const NudfPointCloud* args, void* stream);       /* one thread per occupied cell */
int nudf_pc_thin_round(const NudfPointCloud* args, void* stream);  /* one thread per point */
int nudf_pc_nearest(const NudfPointCloud* args, void* stream);     /* one thread per query */

/* ------------------------------------------------------------------------------------
 * Exact point-to-mesh distance (neuraludf_amd/evaluation.py MeshIndex, closest_on_mesh, mesh_deviation): replaces
 * trimesh.proximity.closest_point, which the reference's users leave the GPU for, and the approximation by a KD-tree on
 * surface samples (sample_mesh + nearest).  The same struct, cell key, hash and ring search as above, over faces binned
 * by their axis-aligned boxes; float64 without contraction, equal to tests/meshdist_ref.py bit for bit.
 *   tribin_count  one thread per face: md_ref_n[f] = the cells of the grid (origin, cell, grid) that the box of face f
 *                 touches, lower corner to upper corner inclusive; 0 for a face with an index outside [0, n_verts) or a
 *                 non-finite coordinate; cap + 1 when more than cap (cap <= 2^40);
 *   tribin_emit   one thread per face: (md_ref_key, md_ref_face)[md_ref_off[f] ...] = (packed cell, f), x outermost.  The
 *                 caller sorts the pairs by key (stable), builds cell_key / cell_start / cell_count over the sorted keys
 *                 and the hash with nudf_pc_cells, and passes the sorted faces as md_cell_face;
 *   closest       one thread per query (cell-sorted for coherence): the closest point of the mesh over the interior and
 *                 the three edges of every face, the smallest (squared distance, face) pair: dist / idx / md_point /
 *                 md_bary [query_idx[t]]; +inf / -1 / NaN / NaN beyond bound.  box_lo / box_hi bound the vertices of the
 *                 binned faces.
 * Host-side refusals (no launch): NULL buffers, cell <= 0 or not finite, a grid axis outside [1, 2^21], n_faces, n_verts
 * or n_query >= 2^31, cap outside [0, 2^40], bound <= 0 (closest).  Empty descriptors return 0.
 * ---------------------------------------------------------------------------------- */
int nudf_pc_tribin_count(const NudfPointCloud* args, void* stream);  /* one thread per face  */
int nudf_pc_tribin_emit(const NudfPointCloud* args, void* stream);   /* one thread per face  */
int nudf_pc_closest(const NudfPointCloud* args, void* stream);       /* one thread per query */

/* ------------------------------------------------------------------------------------
 * Rays against the mesh (neuraludf_amd/evaluation.py MeshIndex.cast, cast_rays, contains_points, signed_distance): replaces
 * trimesh.ray's intersects_first / intersects_any / intersects_location and Trimesh.contains.  The index is the one built
 * for nudf_pc_closest; the struct grew at its end by the md_ray_o ... md_count fields WITHOUT a version step: the version
 * stays 111, and a package and a library that disagree on the size of NudfPointCloud are refused all the same, by the size
 * table of nudf_abi_struct that every loader checks after the version.
 *   raycast       one thread per ray i: walks ray md_ray_o[i] + t md_ray_d[i] through the cells and applies the
 *                 per-(ray, face) rule of DESIGN.md 4.16 (float64 without contraction, equal to tests/meshray_ref.py bit for
 *                 bit; independent of the cell size and of the order of traversal).  md_mode 0: dist / idx / md_bary
 *                 [query_idx[i]] = t, face and barycentric weights of the smallest (t, face) with the three edge functions
 *                 all >= 0 or all <= 0, +inf / -1 / NaN on a miss; 1: md_count[query_idx[i]] = 1 when such a face exists
 *                 (early exit), else 0; 2: md_count = the faces crossed, a zero edge function counting as positive in the
 *                 edge's direction from its lower vertex index to its higher, each face once.
 * Host-side refusals (no launch): NULL buffers, cell <= 0 or not finite, a grid axis outside [1, 2^21], a bad hash_cap,
 * n_faces, n_verts or n_query >= 2^31, an unknown md_mode, md_t_min NaN, md_t_max < md_t_min.  Empty descriptors return 0.
 * ---------------------------------------------------------------------------------- */
int nudf_pc_raycast(const NudfPointCloud* args, void* stream);       /* one thread per ray   */

/* ------------------------------------------------------------------------------------
 * Intersecting faces (neuraludf_amd/evaluation.py MeshIndex.intersections, self_intersections, mesh_intersections;
 * meshclean.drop_self_intersections, close_holes_checked): replaces MeshLab's "select self intersecting faces", libigl's
 * and pymeshfix's tests, which a caller leaves the GPU for.  The index is the one built for nudf_pc_closest.  NO new
 * struct, field or version step: the two entry points read NudfPointCloud's fields as follows.
 *   verts, faces, n_verts, n_faces, origin, cell, grid, box_lo, box_hi, cell_start, cell_count, n_cells, hash_key,
 *   hash_row, hash_cap, md_cell_face, md_n_refs     the indexed mesh, as nudf_pc_closest reads them;
 *   md_mode      0 self: the query triangles are the faces of the indexed mesh (n_query == n_faces, query unused), only
 *                pairs g > t are looked at and faces that share vertices by index follow the shared-vertex rules;
 *                1 two meshes: query [n_query, 3, 3] holds the corner coordinates of the other mesh's triangles;
 *   md_ref_n     [n_query] the pairs of each query triangle (written by isect_count, read by isect_emit);
 *   md_ref_off   [n_query] their exclusive prefix sum (isect_emit);
 *   md_ref_key, md_ref_face, state   [cap] the query triangle, the indexed face and the kind of each pair (isect_emit);
 *   cap          the rows of those three buffers: the total the caller accepted.  A row at or beyond it is not written.
 *   isect_count  one thread per query triangle t: md_ref_n[t] = the pairs it reports (0 for an absent triangle: an index
 *                out of range, a non-finite coordinate);
 *   isect_emit   one thread per query triangle t: its pairs at rows md_ref_off[t] ..., in the order of its walk through
 *                the cells.  The caller sorts them.
 * Both run one device function, without atomics.  Broad phase: t walks the cells its box touches, drops a candidate whose
 * box does not overlap its own (closed, exact) and handles a pair only in the cell that holds the lower corner of the two
 * boxes' intersection: each pair once, whatever the cell size.  Narrow phase (equal to
 * tests/meshintersect_ref.py bit for bit): signs of orient3d / orient2d on input coordinates in Shewchuk's operation
 * order, certified by his stage-A bound ((7 + 56 e) e permanent, (3 + 16 e) e detsum, e = 2^-53; bound > 2^-960), float64
 * without contraction.  The contract: a pair that is not reported is disjoint in exact arithmetic, apart from the shared
 * vertices (the shared edge, where two are shared); a CROSSING pair shares a point in exact arithmetic (one that is not
 * the shared vertex); COPLANAR and UNCERTAIN pairs touch, overlap in a plane or come closer than float64 can tell.
 * Host-side refusals (no launch): NULL buffers, cell <= 0 or not finite, a grid axis outside [1, 2^21], a bad hash_cap,
 * n_faces, n_verts or n_query >= 2^31, an unknown md_mode, n_query != n_faces in self mode, cap < 0.  Empty descriptors
 * (n_query <= 0; for isect_emit also cap == 0) return 0.
 * ---------------------------------------------------------------------------------- */
#define NUDF_ISECT_CROSSING 1   /* the two faces pass through each other                                               */
#define NUDF_ISECT_COPLANAR 2   /* no certified separating edge in the common (or nearly common) plane; a fold        */
#define NUDF_ISECT_UNCERTAIN 3  /* a sign that float64 with the stage-A filter cannot certify                          */
int nudf_pc_isect_count(const NudfPointCloud* args, void* stream);   /* one thread per query triangle */
int nudf_pc_isect_emit(const NudfPointCloud* args, void* stream);    /* one thread per query triangle */

/* ------------------------------------------------------------------------------------
 * Generalised winding numbers (neuraludf_amd/evaluation.py MeshIndex.winding, winding_number, contains_points and
 * signed_distance with method="winding"): inside / outside that survives holes and open sheets; replaces libigl's
 * fast_winding_number, which a caller leaves the GPU for.  NO new struct, field or version step: the three entry points
 * read NudfPointCloud's fields as follows (restated in tests/meshwinding_ref.py).
 *   verts, faces, n_verts, n_faces, origin, cell, grid    the mesh and the leaf grid: origin is the lower corner of the box
 *                of the usable faces, cell the leaf edge, grid the cells per axis (all three entry points check them);
 *   wn_faces     one thread per item t < n_query.  md_mode 0 (n_query == n_faces): keys[t] = the Morton interleave (x the
 *                highest bit of each triple) of the leaf cell of the centroid (p0 + (p1 + p2)) / 3 of face t, clamped into
 *                the grid; -1 for an absent face (an index out of range, a non-finite vertex, an area vector
 *                1/2 (p1 - p0) x (p2 - p0) of zero or non-finite length).  md_mode 1: keys[t] = the key of the cell of point
 *                query[t] (the driver's coherence sort);
 *   md_cell_face, md_n_refs   the usable faces sorted by key (stable) and their number;
 *   n, rank, cell_start, cell_count   the nodes of the linear octree in preorder, rank[i] = skip[i] the first node behind
 *                node i's subtree (a leaf has skip[i] == i + 1), cell_start / cell_count the range of node i's faces in
 *                md_cell_face;
 *   wn_nodes     one thread per node query_idx[t], t < n_query: the nodes of ONE level, the lowest level first.  Writes
 *                out[40 i ...] = the raw moments about origin (W, M[3], S[3], T0[9], Q0[18], box lo[3], hi[3]): a leaf adds
 *                its faces in sorted order, a parent the raw moments of its children in preorder; and md_point[32 i ...] =
 *                the node record (centre[3], r2, S[3], T diagonal[3], T_jk + T_kj[3], Q[18], tr T), moments shifted to
 *                the area-weighted centre;
 *   winding      pts [n, 32] the node records (what wn_nodes wrote through md_point), r2 = beta * beta (>= 1; inf: no node
 *                is ever replaced, the exact sum), query [n_query, 3] / query_idx (NULL: the identity) / n_query the
 *                points.  Writes dist[query_idx[t]] = w, and where the pointers are not NULL md_count[...] = the faces
 *                evaluated exactly and idx[...] = the nodes replaced by their expansion.  One wavefront walks the preorder
 *                for its 64 queries together with a wave-uniform node index; per query the result is that of the
 *                single-query walk, bit for bit.
 * No atomics, no LDS, no scratch memory.  Float64 without contraction; only atan2 is not defined to the bit.
 * Host-side refusals (no launch): NULL buffers, cell <= 0 or not finite, a grid axis outside [1, 2^21], a non-finite
 * origin, n_query, n_faces, n_verts, n or md_n_refs >= 2^31, an unknown md_mode or n_query != n_faces (wn_faces), no
 * nodes or no faces (wn_nodes, winding), beta * beta < 1 or NaN (winding).  Empty descriptors (n_query <= 0) return 0.
 * ---------------------------------------------------------------------------------- */
int nudf_pc_wn_faces(const NudfPointCloud* args, void* stream);      /* one thread per face (or point) */
int nudf_pc_wn_nodes(const NudfPointCloud* args, void* stream);      /* one thread per node of a level */
int nudf_pc_winding(const NudfPointCloud* args, void* stream);       /* one wavefront per 64 queries   */

/* ------------------------------------------------------------------------------------
 * Mesh topology for the mesh clean-up (neuraludf_amd/meshclean.py): replaces what the reference does with trimesh,
 * networkx, scipy.sparse and cv2 on the CPU -- trimesh's fill_holes (extract_mesh.py:222-223), the border smoothing
 * (extract_mesh.py:238-265), clean_mesh_by_faces_num / clean_outliers (evaluation/clean_dtu_mesh.py:158-191) and
 * clean_points_by_mask / clean_points_by_visualhull (clean_dtu_mesh.py:36-105).  One struct; each entry point reads the
 * fields its comment names.  Half-edge 3 f + k of face f runs faces[f][k] -> faces[f][(k + 1) % 3]; its key is
 * min * n_verts + max (n_verts < 2^31).  The caller sorts the keys (stable) and scans between launches.
 *   edges       one thread per unique edge e: edges[e] = (u, v, count, first face, second face or -1) with u <= v, and
 *               he_edge[h] = e for each of its half-edges;
 *   fill_count  one thread per boundary vertex i: new_count[i] = triangles of the hole whose smallest vertex bverts[i]
 *               is (a closed loop of 3 or 4 <= max_loop boundary edges whose vertices all have boundary degree 2; a 3-loop
 *               whose triangle exists gets none);
 *   fill_emit   the same walk; writes the triangles at new_faces[new_off[i]...].  A 4-loop is split along the shorter
 *               diagonal (float64 squared length, tie: through the smallest vertex).  A triangle starts at its smallest
 *               vertex and ascends, unless more of its boundary edges run in that same direction in their face than
 *               against it;
 *   smooth      one thread per border vertex v: pos_out[v] = pos[v] + lam (mean of pos over v's boundary neighbours, in
 *               ascending index - pos[v]), float64;
 *   cc_hook     one thread per sorted half-edge j >= 1 whose key equals that of j - 1: the larger of the two faces' roots
 *               takes the smaller as label (atomicMin), *changed = 1;
 *   cc_jump     one thread per face: labels[f] = its root.  Rounds of hook + jump until *changed stays 0 end with
 *               labels[f] = the smallest face index of f's component;
 *   views       one thread per vertex: vis_count[v] = views i with round-half-even((proj_i p)_xy / (proj_i p)_z) + 1 inside
 *               [border, W - border] x [border, H - border] and the mask, padded by one pixel of ones, set there.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfMeshTopo {
  const int64_t* faces;      /* [n_faces, 3]                                                                         */
  const int64_t* he_key;     /* [3 n_faces] half-edge keys, ascending (edges, cc_hook)                               */
  const int64_t* he_id;      /* [3 n_faces] the half-edge at each sorted position (edges, cc_hook)                   */
  const int64_t* edge_start; /* [n_edges] sorted position of the first half-edge of each unique edge (edges)         */
  int64_t* edges;            /* [n_edges, 5] (edges: written; fill_*: read)                                          */
  int64_t* he_edge;          /* [3 n_faces] (edges)                                                                  */
  const int64_t* edge_key;   /* [n_edges] the unique keys, ascending (fill_*)                                        */
  const int64_t* nbr_off;    /* [n_verts + 1] CSR of the boundary neighbours (fill_*, smooth)                        */
  const int64_t* nbr;        /* boundary neighbours of each vertex, ascending (fill_*, smooth)                       */
  const int64_t* bverts;     /* [n_bverts] the vertices with a boundary edge, ascending (fill_*, smooth)             */
  int64_t* new_count;        /* [n_bverts] (fill_count)                                                              */
  const int64_t* new_off;    /* [n_bverts] exclusive prefix sum of new_count (fill_emit)                             */
  int64_t* new_faces;        /* [n_new, 3] (fill_emit)                                                               */
  const double* pos;         /* [n_verts, 3] vertex positions (fill_emit, smooth, views)                             */
  double* pos_out;           /* [n_verts, 3] (smooth; only the rows of bverts are written)                           */
  int64_t* labels;           /* [n_faces] set to 0 .. n_faces - 1 by the caller (cc_*)                               */
  int32_t* changed;          /* one word, zeroed by the caller before each round (cc_hook)                           */
  const double* proj;        /* [n_views, 3, 4] rows 0..2 of each world matrix (views)                               */
  const uint8_t* masks;      /* [n_views, H, W] non-zero = set (views)                                               */
  int32_t* vis_count;        /* [n_verts] (views)                                                                    */
  int64_t n_faces;
  int64_t n_verts;
  int64_t n_edges;
  int64_t n_bverts;
  int64_t n_new;
  double lam;                /* smooth: the step, 0.3 in the reference                                               */
  int32_t max_loop;          /* fill_*: 3 or 4                                                                       */
  int32_t n_views;
  int32_t H;
  int32_t W;
  int32_t border;            /* views: 0 for the mask test, 50 for the visual-hull test                              */
  int32_t pad_;
  /* mesh simplification (nudf_meshsimplify_*, below); `pos`, `faces`, `edges`, `he_edge`, n_faces, n_verts and n_edges
   * above are read too */
  int64_t* sp_key;               /* [n_verts] (keys)                                                                 */
  const int64_t* sp_cluster_key; /* [n_clusters] the unique keys, ascending (place)                                  */
  const int64_t* sp_vcluster;    /* [n_verts] cluster of each vertex = rank of its key (faces)                       */
  const int64_t* sp_member_off;  /* [n_clusters + 1] CSR offsets of the member vertices (place)                      */
  const int64_t* sp_member;      /* [n_verts] the vertices grouped by cluster, ascending inside each (place)         */
  const int64_t* sp_corner_off;  /* [n_clusters + 1] CSR offsets of the corners (place, sp_placement 0)              */
  const int64_t* sp_corner;      /* [3 n_faces] the corners 3 f + k grouped by cluster, ascending inside each (place) */
  const double* sp_attr;         /* [n_verts, sp_attr_width] vertex attributes, or NULL with width 0 (place)         */
  double* sp_rep;                /* [n_clusters, 3] the representatives (place)                                      */
  uint8_t* sp_accepted;          /* [n_clusters] 1: the quadric solution was taken, 0: the mean (place)              */
  double* sp_quadric;            /* [n_clusters, 10] A00 A01 A02 A11 A12 A22 b0 b1 b2 c, or NULL: not stored (place) */
  double* sp_attr_out;           /* [n_clusters, sp_attr_width] attribute means (place)                              */
  int64_t* sp_faces;             /* [n_faces, 3] the faces over cluster ids (faces)                                  */
  int64_t* sp_triple;            /* [n_faces, 3] the same ids in ascending order (faces)                             */
  uint8_t* sp_degenerate;        /* [n_faces] 1: two corners share a cluster (faces)                                 */
  int64_t n_clusters;
  int64_t sp_grid[3];            /* cells per axis, each in [1, 2^20]                                                */
  double sp_origin[3];           /* the corner of cell (0, 0, 0)                                                     */
  double sp_cell;                /* edge length of a cell, > 0                                                       */
  double sp_lambda;              /* place: the regularisation, > 0                                                   */
  double sp_boundary_weight;     /* place: weight of the boundary planes relative to their faces'; 0: none, and      */
                                 /* edges / he_edge are not read                                                     */
  int32_t sp_attr_width;
  int32_t sp_placement;          /* place: 0 quadric, 1 mean (no corner walk, sp_accepted all 0)                     */
  /* subdivision (nudf_meshsubdiv_*, below), appended WITHOUT a version step.  The prefix is sp_sd_ because the tests of
   * the simplification pin that every field after pad_ is named sp_... (or n_clusters); `faces`, `edges`, `he_edge`,
   * `he_id`, `edge_start`, `nbr_off` / `nbr`, `pos`, sp_attr, sp_attr_width, n_faces, n_verts and n_edges are read too */
  uint8_t* sp_sd_mark;               /* [n_edges] 1: the edge is split (mark)                                        */
  const int64_t* sp_sd_edge_vertex;  /* [n_edges] n_verts + rank among the marked edges, or -1 (count, emit)         */
  const int64_t* sp_sd_marked;       /* [sp_sd_n_marked] the marked edges, ascending (odd)                           */
  const int64_t* sp_sd_ring_off;     /* [n_verts + 1] CSR offsets of the one-rings (even, scheme 1)                  */
  const int64_t* sp_sd_ring;         /* [sp_sd_n_ring] the one-ring of each vertex, ascending (even, scheme 1)       */
  const uint8_t* sp_sd_vclass;       /* [n_verts] 0 smooth, 1 border, 2 stays (even, scheme 1)                       */
  double* sp_sd_pos_out;             /* [n_verts + sp_sd_n_marked, 3] (even: the first n_verts rows, odd: the rest;  */
                                     /* emit reads it)                                                               */
  double* sp_sd_attr_out;            /* [n_verts + sp_sd_n_marked, sp_attr_width], rows as in sp_sd_pos_out          */
  int64_t* sp_sd_fcount;             /* [n_faces] children of each face (count)                                      */
  const int64_t* sp_sd_foff;         /* [n_faces] exclusive prefix sum of sp_sd_fcount (emit)                        */
  int64_t* sp_sd_faces_out;          /* [sp_sd_n_out, 3] (emit)                                                      */
  int64_t* sp_sd_parent;             /* [sp_sd_n_out] the input face of each output face (emit)                      */
  int64_t sp_sd_n_ring;
  int64_t sp_sd_n_border;            /* entries of `nbr` (even, scheme 1)                                            */
  int64_t sp_sd_n_marked;
  int64_t sp_sd_n_out;
  double sp_sd_max_edge;             /* mark: > 0 and finite unless sp_sd_mark_all                                   */
  int32_t sp_sd_scheme;              /* odd, even: 0 midpoint, 1 loop                                                */
  int32_t sp_sd_mark_all;            /* mark: non-zero marks every edge with u != v                                  */
  /* hole closing (nudf_meshhole_*, below), appended WITHOUT a version step; the prefix stays sp_sd_ for the reason above.
   * Read too, in their first meaning: `faces`, `edges`, `he_edge`, `edge_key`, `pos`, n_faces, n_verts, n_edges.  Reused
   * with the item changed from a boundary vertex to a loop: new_count [sp_sd_hf_n_loops] the triangles of each loop
   * (count), new_off their exclusive prefix sum (triangulate), new_faces [n_new, 3] and n_new (triangulate), and
   * max_loop, here the longest loop that is closed, 3 ... NUDF_HOLE_MAX_EDGES (count, triangulate).  `labels`,
   * `changed`, `nbr*` and `bverts` are not reused: a state's label travels with its jump and distance in one row of
   * sp_sd_hf_rank_*, no round reports a change, and the border here is a list of edges, not of vertices */
  const int64_t* sp_sd_hf_bedge;     /* [sp_sd_hf_n_border] the rows of `edges` with count 1, ascending (link)       */
  const int64_t* sp_sd_hf_brank;     /* [n_edges] position of the edge in sp_sd_hf_bedge, or -1 (link)               */
  int64_t* sp_sd_hf_link;            /* [2 sp_sd_hf_n_border] partner of state 2 b + end, or -1 (link)               */
  const int64_t* sp_sd_hf_rank_in;   /* [2 sp_sd_hf_n_border, 3] (jump, smallest state id, distance to it) (rank)    */
  int64_t* sp_sd_hf_rank_out;        /* [2 sp_sd_hf_n_border, 3] the same after the round; not sp_sd_hf_rank_in      */
  const int64_t* sp_sd_hf_loop_off;  /* [sp_sd_hf_n_loops + 1] CSR offsets of the loops (count, triangulate)         */
  const int64_t* sp_sd_hf_loop_vertex; /* [sp_sd_hf_n_items] vertex at which each edge is entered (count, triangulate) */
  const int64_t* sp_sd_hf_loop_edge; /* [sp_sd_hf_n_items] the rows of `edges` in loop order (count, triangulate)    */
  const uint8_t* sp_sd_hf_closed;    /* [sp_sd_hf_n_loops] 1: a closed loop, 0: a chain between blocked ends (count) */
  double* sp_sd_hf_perimeter;        /* [sp_sd_hf_n_loops] (count)                                                   */
  int8_t* sp_sd_hf_status;           /* [sp_sd_hf_n_loops] NUDF_HOLE_ (count: written; triangulate: read, and        */
                                     /* NUDF_HOLE_DUPLICATE written for a refused loop)                              */
  int64_t sp_sd_hf_n_border;
  int64_t sp_sd_hf_n_loops;
  int64_t sp_sd_hf_n_items;          /* entries of sp_sd_hf_loop_vertex / _edge: sp_sd_hf_n_border for a full table  */
  double sp_sd_hf_max_perimeter;     /* count: > 0; +inf for no bound                                                */
  int32_t sp_sd_hf_round;            /* rank: the round r = 0, 1, ...: the spans read are 2^r states long            */
  int32_t sp_sd_hf_pad_;
  /* isotropic remeshing (nudf_meshremesh_*, below), appended WITHOUT a version step; the prefix grows to sp_sd_hf_rm_
   * because the tests of the hole closing pin that every field after the subdivision's is named sp_sd_hf_...  Read too, in
   * their first meaning: `faces`, `edges`, `he_edge`, `he_id`, `edge_start`, `edge_key`, `pos`, `nbr_off` / `nbr` with
   * sp_sd_n_border (the border neighbours), sp_sd_ring_off / sp_sd_ring with sp_sd_n_ring (the one-rings), sp_sd_vclass,
   * n_faces, n_verts, n_edges */
  const int64_t* sp_sd_hf_rm_corner_off; /* [n_verts + 1] CSR offsets of the corners (collapse_check, vertex_min 2)  */
  const int64_t* sp_sd_hf_rm_corner;     /* [3 n_faces] the corners 3 f + k by vertex, ascending inside each         */
  const int64_t* sp_sd_hf_rm_vedge_off;  /* [n_verts + 1] CSR offsets of the incident edges (vertex_min 0, relax)    */
  const int64_t* sp_sd_hf_rm_vedge;      /* [sp_sd_hf_rm_n_vedge] the rows of `edges` at each vertex                 */
  uint8_t* sp_sd_hf_rm_status;           /* [n_edges] NUDF_REMESH_ (the checks: written; vertex_min, apply: read)    */
  int64_t* sp_sd_hf_rm_keep;             /* [n_edges] the end that stays, or -1 (collapse_check; collapse_apply reads) */
  int64_t* sp_sd_hf_rm_gone;             /* [n_edges] the end that goes, or -1                                       */
  int32_t* sp_sd_hf_rm_gain;             /* [n_edges] fall of the squared valence deviation (flip_check)             */
  int64_t* sp_sd_hf_rm_ab;               /* [n_edges, 2] the corners opposite the edge, or -1 (flip_check; flip_apply reads) */
  const int64_t* sp_sd_hf_rm_rank;       /* [n_edges] place among the candidates, n_edges for none (vertex_min, apply) */
  const int64_t* sp_sd_hf_rm_best_in;    /* [n_verts] (vertex_min 1; the apply kernels: the last pass's output)      */
  int64_t* sp_sd_hf_rm_best_out;         /* [n_verts] (vertex_min); not sp_sd_hf_rm_best_in                          */
  int64_t* sp_sd_hf_rm_remap;            /* [n_verts] preset to the identity (collapse_apply: the rows of the ends that go) */
  double* sp_sd_hf_rm_pos_out;           /* [n_verts, 3] preset to a copy of pos (collapse_apply: the rows of the ends */
                                         /* that stay; relax: every row)                                             */
  int64_t* sp_sd_hf_rm_faces_out;        /* [n_faces, 3] preset to a copy of faces (flip_apply: the winners' two rows) */
  uint8_t* sp_sd_hf_rm_win;              /* [n_edges] 1: the edge was collapsed / flipped (the apply kernels)        */
  int64_t sp_sd_hf_rm_n_vedge;
  double sp_sd_hf_rm_low;                /* collapse_check: an edge shorter than this is collapsed; > 0 and finite   */
  double sp_sd_hf_rm_high;               /* collapse_check: no edge longer than this is made; > 0 and finite         */
  double sp_sd_hf_rm_cos_border;         /* collapse_check: cosine of the largest turn of the border that is removed */
  int32_t sp_sd_hf_rm_mode;              /* vertex_min: 0 edges at the vertex, 1 the one-ring, 2 edges of the faces  */
  int32_t sp_sd_hf_rm_pad_;
} NudfMeshTopo;
int nudf_meshtopo_edges(const NudfMeshTopo* args, void* stream);       /* one thread per unique edge      */
int nudf_meshtopo_fill_count(const NudfMeshTopo* args, void* stream);  /* one thread per boundary vertex  */
int nudf_meshtopo_fill_emit(const NudfMeshTopo* args, void* stream);   /* one thread per boundary vertex  */
int nudf_meshtopo_smooth(const NudfMeshTopo* args, void* stream);      /* one thread per boundary vertex  */
int nudf_meshtopo_cc_hook(const NudfMeshTopo* args, void* stream);     /* one thread per sorted half-edge */
int nudf_meshtopo_cc_jump(const NudfMeshTopo* args, void* stream);     /* one thread per face             */
int nudf_meshtopo_views(const NudfMeshTopo* args, void* stream);       /* one thread per vertex           */

/* ------------------------------------------------------------------------------------
 * Mesh simplification (neuraludf_amd/meshclean.py simplify_mesh, simplify_to_faces): vertex clustering on a uniform grid
 * with each cluster's representative placed by quadric error minimisation.  The reference has no such step: its users
 * take the mesher's output, whose triangles are as small as the grid spacing, to trimesh or open3d on the CPU.  The entry
 * points take NudfMeshTopo and read the sp_ fields at its end.  The caller sorts the keys and the corners' clusters
 * (stable) and scans between the launches; float64 without contracted multiply-adds, every sum in list order inside one
 * thread, no atomics: every result is identical from run to run.
 *   keys    one thread per vertex: c = floor((pos[v] - sp_origin) / sp_cell) per axis and
 *           sp_key[v] = (cx Gy + cy) Gz + cz in int64 with G = sp_grid; -1 when a coordinate is not finite or c lies
 *           outside [0, G) (the caller raises).  Clusters are the unique keys in ascending order;
 *   place   one thread per cluster.  Coordinates are local to the cell's centre, sp_origin + (c + 1/2) sp_cell.  The mean
 *           is the sum of (pos[v] - centre) over the members in list order divided by their number.  With sp_placement 0
 *           the quadric (A, b, c) is summed over the cluster's corners in list order: corner (f, k) adds the plane of its
 *           face -- n = (p1 - p0) x (p2 - p0), u = n / |n|, w = |n| / 2, d = -u . (p0 - centre), the plane adding
 *           (w u u^T, (w d) u, (w d) d) -- then, with sp_boundary_weight != 0, the boundary plane of half-edge 3 f + k and
 *           then that of half-edge 3 f + (k + 2) % 3 (the one that ends at the corner), each only when
 *           edges[he_edge[h]].count is 1: for half-edge j with e = p_{j+1} - p_j and m = e x u, the plane through p_j with
 *           normal m / |m| and weight sp_boundary_weight * w.  A face whose |n| is 0 or not finite adds nothing, as does a
 *           boundary plane whose |m| is.  With t = A00 + A11 + A22 > 0, (A + lambda t I) x = -b + lambda t mean is solved
 *           by a Cholesky factorisation without pivoting (the matrix is positive definite with condition at most
 *           (1 + lambda) / lambda), and x is taken exactly when the key of centre + x, computed as in `keys`, is the
 *           cluster's; otherwise, and with sp_placement 1, the mean.  sp_rep[c] = centre + x or centre + mean,
 *           sp_accepted[c] says which, sp_quadric[c] (when not NULL) holds the ten sums, and sp_attr_out[c] the mean of
 *           each attribute column over the members in list order;
 *   faces   one thread per face: sp_faces[f] = the clusters of its corners, sp_degenerate[f] = two of them are equal,
 *           sp_triple[f] = the three in ascending order.  Of the faces with equal triples the caller keeps the one with the
 *           smallest index.
 * ---------------------------------------------------------------------------------- */
int nudf_meshsimplify_keys(const NudfMeshTopo* args, void* stream);    /* one thread per vertex           */
int nudf_meshsimplify_place(const NudfMeshTopo* args, void* stream);   /* one thread per cluster          */
int nudf_meshsimplify_faces(const NudfMeshTopo* args, void* stream);   /* one thread per face             */

/* ------------------------------------------------------------------------------------
 * Mesh subdivision (neuraludf_amd/meshclean.py subdivide_mesh, subdivide_to_edge): Loop and midpoint subdivision and
 * splitting of the edges longer than a bound.  The reference has no such step: its users take the mesh to
 * trimesh.remesh.subdivide / subdivide_loop / subdivide_to_size or open3d on the CPU.  The entry points take NudfMeshTopo
 * and read the sp_sd_ fields at its end (no version step: the size table of nudf_abi_struct refuses a package and a library
 * that disagree).  An edge is a row of `edges`.  The caller ranks the marked edges and scans the face counts between the
 * launches; float64 without contracted multiply-adds, every sum in list order inside one thread, no atomics: every result
 * is identical from run to run and equals tests/meshsubdiv_ref.py bit for bit.
 *   mark    one thread per edge (u, v): sp_sd_mark[e] = u != v && (sp_sd_mark_all || (dx dx + dy dy) + dz dz >
 *           sp_sd_max_edge sp_sd_max_edge), d = pos[u] - pos[v]; a NaN length is not marked.  The new vertex of the j-th
 *           marked edge is n_verts + j: the output vertices are the old ones followed by one per marked edge;
 *   odd     one thread per marked edge: row n_verts + j of sp_sd_pos_out.  Scheme 0: (p_u + p_v) 0.5.  Scheme 1: an edge
 *           with exactly two half-edges h0 = he_id[edge_start[e]] and h1 = he_id[edge_start[e] + 1] gets
 *           (p_u + p_v) 0.375 + (p_a + p_b) 0.125, a and b = faces[h / 3][(h % 3 + 2) % 3] of h0 and h1; every other
 *           edge is a crease and gets the midpoint;
 *   even    one thread per old vertex: row v of sp_sd_pos_out.  Scheme 0: a copy.  Scheme 1: class 2 stays; class 1, with
 *           exactly two border neighbours b0 <= b1 in `nbr`, moves to p 0.75 + (p_b0 + p_b1) 0.125; class 0 with a
 *           one-ring of n > 0 vertices moves to p (1 - n beta) + s beta, beta = 3 / 16 for n = 3 and 3 / (8 n) otherwise,
 *           s the sum of the ring in list order starting from its first entry; anything else stays.  The caller sets
 *           class 2 for a vertex on an edge with three or more half-edges or with a number of border edges other than 0
 *           and 2, class 1 for one with two border edges;
 *   count   one thread per face: sp_sd_fcount[f] = 1 + its marked half-edges;
 *   emit    one thread per face, children at sp_sd_foff[f] in the parent's winding, m_k the new vertex of half-edge
 *           k (v_k -> v_k+1):  none marked: (v0, v1, v2);  one, k, with (a, b, c) = (v_k, v_k+1, v_k+2): (a, m, c),
 *           (m, b, c);  two, k unmarked, (a, b, c) as before, m1 = m_k+1, m2 = m_k+2: (m1, c, m2), then the quad
 *           a b m1 m2 along the shorter of a-m1 and b-m2 (squared float64 lengths in sp_sd_pos_out, on a tie a-m1 exactly
 *           when a < b): (a, b, m1), (a, m1, m2) or (a, b, m2), (b, m1, m2);  three: (v0, m0, m2), (m0, v1, m1),
 *           (m2, m1, v2), (m0, m1, m2).  sp_sd_parent[i] = f for each child i.
 * sp_attr columns go through the weights of the positions into sp_sd_attr_out.  An index read from a table that is out
 * of range makes its item a copy (odd: a zero row; emit: nothing written); nothing is addressed outside the buffers.
 * Host-side refusals (no launch): negative counts, n_verts + sp_sd_n_marked >= 2^31, n_faces >= 2^31, NULL buffers,
 * sp_sd_max_edge not positive and finite without sp_sd_mark_all, an unknown sp_sd_scheme.  Empty jobs return 0.
 * ---------------------------------------------------------------------------------- */
int nudf_meshsubdiv_mark(const NudfMeshTopo* args, void* stream);      /* one thread per unique edge      */
int nudf_meshsubdiv_odd(const NudfMeshTopo* args, void* stream);       /* one thread per marked edge      */
int nudf_meshsubdiv_even(const NudfMeshTopo* args, void* stream);      /* one thread per vertex           */
int nudf_meshsubdiv_count(const NudfMeshTopo* args, void* stream);     /* one thread per face             */
int nudf_meshsubdiv_emit(const NudfMeshTopo* args, void* stream);      /* one thread per face             */

/* ------------------------------------------------------------------------------------
 * Hole closing (neuraludf_amd/meshclean.py border_loops, close_holes): the border loops of a mesh, defined through the
 * fans of its surface, and the minimum-area triangulation of those of up to NUDF_HOLE_MAX_EDGES edges (Barequet and
 * Sharir 1995; the area term of Liepa's weight).  nudf_meshtopo_fill_* mirror trimesh's fill_holes and stop at 4 edges;
 * the reference's users take longer holes to MeshLab or pymeshfix on the CPU.  The entry points take NudfMeshTopo and
 * read the sp_sd_hf_ fields at its end (no version step, as for the subdivision).  The caller sorts and scans between the
 * launches; float64 without contracted multiply-adds, every sum in list order inside one thread, no atomics: every
 * result is identical from run to run and equals tests/meshhole_ref.py bit for bit.
 * A border edge is a row of `edges` with count 1; border edge b = sp_sd_hf_bedge[b] has the ends 0 (its u) and 1 (its v),
 * and state 2 b + end names the pair.
 *   link         one thread per state: the fan walk around v, the vertex at that end.  It starts in the edge's face and
 *                steps across the face's other edge at v into the neighbouring face for as long as that edge has count 2;
 *                at the first edge of another count it ends: count 1 is the linked border edge b', and
 *                sp_sd_hf_link[s] = 2 b' + (the end of b' that is v); count 3 and more is a blocked end, -1.  Blocked
 *                too: a face with a repeated vertex (the first included), a walk that returns to its first face, more
 *                than NUDF_HOLE_FAN_CAP faces, a linked edge with u = v.  The link pairs the states and does not look at
 *                the winding; the border edges fall into closed loops and into chains between two blocked ends;
 *   rank         one thread per directed state (2 b + the end the edge is entered by), one pointer-doubling round r:
 *                with (j, m, d) = sp_sd_hf_rank_in[s] and (j', m', d') = sp_sd_hf_rank_in[j], sp_sd_hf_rank_out[s] =
 *                (j', m', 2^r + d') when m' < m, else (j', m, d); a j outside [0, 2 sp_sd_hf_n_border) copies the row.
 *                The caller starts from (succ(s), s, 0), succ(s) = link[s ^ 1] (across the edge, then along the link) or,
 *                at a blocked end, s ^ 1 (back along the chain: a chain of n edges is a cycle of 2 n states, a loop two
 *                cycles of n, one per direction), and runs ceil(log2(2 B)) + 1 rounds between two buffers: then m is the
 *                smallest state of the cycle and d the steps to it;
 *   count        one thread per loop l of the CSR sp_sd_hf_loop_off: sp_sd_hf_perimeter[l] = the lengths
 *                sqrt((dx dx + dy dy) + dz dz), d = pos[u] - pos[v], of its edges summed in loop order from the first;
 *                sp_sd_hf_status[l] = the first that holds of NUDF_HOLE_OPEN_CHAIN (sp_sd_hf_closed[l] is 0),
 *                _TOO_MANY_EDGES (more than max_loop), _REPEATED_VERTEX (a vertex twice in sp_sd_hf_loop_vertex),
 *                _NONFINITE (a coordinate of a loop vertex or the perimeter), _PERIMETER (perimeter >
 *                sp_sd_hf_max_perimeter), else _FILLED; new_count[l] = n - 2 for _FILLED, else 0;
 *   triangulate  one wavefront per loop with status _FILLED and vertices v_0 ... v_n-1.  W[i][i + 1] = 0 and, diagonal
 *                by diagonal d = j - i = 2 ... n - 1 with the cells of one across the lanes, W[i][j] = the minimum over
 *                i < k < j of (W[i][k] + W[k][j]) + A(i, k, j), A = 0.5 sqrt(|(v_k - v_i) x (v_j - v_i)|^2); k ascends
 *                and only a strictly smaller value replaces the first, split[i][j] = that k.  W, split and the positions
 *                live in LDS (under 40 KB for the workgroup).  One lane lists the n - 2 triangles (i, k, j) in pre-order
 *                from (0, n - 1): the triangle, then (i, k), then (k, j).  Every chord (i, j) of that list but the
 *                root's is a diagonal and is looked up in edge_key; if one is an edge already, or for n = 3 when the three
 *                border edges have one and the same face, the loop is refused whole: status _DUPLICATE and its rows of
 *                new_faces set to -1.  Otherwise row new_off[l] + t is (v_i, v_k, v_j) of triangle t, or (v_i, v_j, v_k)
 *                when more than half of the loop's border edges run, in the face next to them, in loop direction: the
 *                patch runs against the majority of its neighbours and keeps the loop's direction on a tie.
 * An index read from a table that is out of range blocks the end (link), copies the row (rank), gives status _NONFINITE
 * and a NaN perimeter (count) or leaves the loop's rows as they were (triangulate); nothing is addressed outside the
 * buffers.  Host-side refusals (no launch): negative counts, counts above their bound (sp_sd_hf_n_border <= n_edges;
 * sp_sd_hf_n_loops, sp_sd_hf_n_items, n_new <= sp_sd_hf_n_border), NULL buffers, max_loop outside
 * [3, NUDF_HOLE_MAX_EDGES], a sp_sd_hf_max_perimeter that is not positive, a round outside [0, 40], equal rank buffers.
 * Empty jobs return 0.
 * ---------------------------------------------------------------------------------- */
#define NUDF_HOLE_MAX_EDGES 64
#define NUDF_HOLE_FAN_CAP 4096
enum {
  NUDF_HOLE_FILLED = 0,
  NUDF_HOLE_OPEN_CHAIN = 1,
  NUDF_HOLE_TOO_MANY_EDGES = 2,
  NUDF_HOLE_PERIMETER = 3,
  NUDF_HOLE_NONFINITE = 4,
  NUDF_HOLE_DUPLICATE = 5,
  NUDF_HOLE_REPEATED_VERTEX = 6
};
int nudf_meshhole_link(const NudfMeshTopo* args, void* stream);        /* one thread per (border edge, end) */
int nudf_meshhole_rank(const NudfMeshTopo* args, void* stream);        /* one thread per directed state     */
int nudf_meshhole_count(const NudfMeshTopo* args, void* stream);       /* one thread per loop               */
int nudf_meshhole_triangulate(const NudfMeshTopo* args, void* stream); /* one wavefront per loop            */

/* ------------------------------------------------------------------------------------
 * Isotropic remeshing (neuraludf_amd/meshclean.py remesh_isotropic): the loop of Botsch and Kobbelt, "A remeshing approach
 * to multiresolution modeling" (2004) -- split the long edges (nudf_meshsubdiv_*), collapse the short ones, flip towards
 * valence 6, relax tangentially, project (nudf_pc_closest).  The reference has no such step: its users take the mesh to
 * pymeshlab, CGAL or trimesh.remesh on the CPU.  The entry points take NudfMeshTopo and read the sp_sd_hf_rm_ fields at
 * its end (no version step, as for the subdivision).  The caller sorts, ranks and compacts between the launches; float64
 * without contracted multiply-adds, every sum in list order inside one thread, no atomics: every result is identical
 * from run to run and equals tests/meshremesh_ref.py bit for bit.
 * An edge is a row (u, v, count, ...) of `edges`, u < v.  The class of a vertex is sp_sd_vclass (0 smooth, 1 border with
 * exactly two border edges, 2 stays), its valence the length of its one-ring, its target valence 6 (class 0) or 4 (class
 * 1).  A face's normal is (p1 - p0) x (p2 - p0) with the corners rotated so that the smallest vertex index comes first:
 * no bit of it depends on where the face's list starts, and reversing the face negates it exactly.  A status is the first
 * NUDF_REMESH_ code that applies, in the order of the text.
 *   collapse_check  one thread per edge: sp_sd_hf_rm_status, _keep, _gone (-1 unless a candidate).  _COUNT: count is
 *                   neither 1 nor 2, or u = v.  _LONG: not (dx dx + dy dy) + dz dz < low low (a NaN fails).  _CLASS: an
 *                   end of class 2.  Then for count 2: _BORDER when both ends are of class 1; with one such end it is
 *                   kept and stays where it is, with none u is kept and moves to (p_u + p_v) 0.5.  For count 1 the ends
 *                   are tried in the order (keep u, remove v), (keep v, remove u); the removed end g with its other
 *                   border neighbour o (from `nbr`) must have cos_border < 1 and (p_g - p_o) . (p_k - p_g) >
 *                   (cos_border |p_g - p_o|) |p_k - p_g| (the corners of the border stay; a cosine of 1 keeps every
 *                   border vertex), and o must not be the corner opposite the edge (an ear would take a second border
 *                   edge with it); the kept end stays where it is; _BORDER when neither order passes.  _LINK: the merge
 *                   of the two ascending one-rings does not find exactly `count` common vertices.  _CLASS again: the
 *                   one-ring of the removed end holds a vertex of class 2 (such a vertex keeps its faces).  _REACH: a vertex x of
 *                   either one-ring other than u and v with not |p_x - p_new|^2 <= high high.  _FOLD: a face at u or v
 *                   (corner lists) that does not hold both ends with not n_old . n_new > 0, n_new with both ends at
 *                   p_new (independent of the winding; a NaN fails).  _DUPLICATE (count 2): with a, b the corners
 *                   opposite the edge, the faces (u, a, b) and (v, a, b) both exist and would become one.  For count 1
 *                   the order that first passes _CLASS, _REACH, _FOLD is taken; if none does the status is that of the first
 *                   order whose border test passed;
 *   vertex_min      one thread per vertex w, into sp_sd_hf_rm_best_out.  Mode 0: the smallest sp_sd_hf_rm_rank among the
 *                   candidate edges (status 0) in w's list of sp_sd_hf_rm_vedge.  Mode 1: the minimum of
 *                   sp_sd_hf_rm_best_in over w and its one-ring.  Mode 2: the smallest rank among the candidate edges
 *                   that are one of the three edges (he_edge) of a face at w: the edges at w and those opposite it.
 *                   "None" is n_edges.  The ranks are the caller's, a stable sort over the candidates: squared length
 *                   ascending, then edge index (collapse); gain descending, then edge index (flip);
 *   collapse_apply  one thread per edge: a candidate wins exactly when rank[e] = min(best_in[u], best_in[v]); it writes
 *                   remap[gone] = keep, row keep of pos_out and win[e] = 1 (0 for every other edge).  With best_in =
 *                   mode 0 followed by k passes of mode 1, best_in[u] is the smallest rank of a candidate with an end
 *                   within k edges of u, so a winner e = (u, v) has the smallest rank of all candidates with an end
 *                   within k edges of u or v.  If a second winner e' had an end x within k edges of u, then rank[e] <=
 *                   rank[e'], and as u is within k edges of x also rank[e'] <= rank[e]: e' = e.  A collapse reads the
 *                   one-rings of u and v and reads and changes only the faces at u and v; with k = 1 no winner has an
 *                   end in N[u] + N[v] of another (closed neighbourhoods), so no face is at the ends of two winners and
 *                   no vertex a winner reads moves; with k = 2, which the driver uses, N[u] + N[v] of two winners share
 *                   no vertex at all.  The caller maps `faces` through remap and drops the faces with two equal corners;
 *   flip_check      one thread per edge: status, sp_sd_hf_rm_gain, sp_sd_hf_rm_ab.  _COUNT: count is not 2, or u = v.
 *                   With h0 = he_id[edge_start[e]], h1 the next, a and b the corners opposite h0 and h1 -- _SAME: a = b,
 *                   or one of them is u or v.  _CLASS: one of u, v, a, b is of class 2.  _EXISTS: min(a, b) n_verts +
 *                   max(a, b) is in edge_key.  _GAIN: not gain > 0, gain = the sum of (valence - target)^2 over the four
 *                   minus the same with u and v one lower and a and b one higher.  _FOLD: child 0 is face(h0) with v
 *                   replaced by b, child 1 face(h1) with u replaced by a (each keeps its parent's winding; the two
 *                   children do not depend on the winding of either parent); with n0, n1 the parents' normals, m0, m1 the
 *                   children's and c = +1 when h0 and h1 run against each other (the faces are wound alike), else -1,
 *                   all of m0 . n0, m1 . n1, c (m0 . n1), c (m1 . n0) must be > 0;
 *   flip_apply      one thread per edge: a candidate wins when rank[e] = best_in[x] (mode 2) for all four of u, v, a, b:
 *                   e is an edge of a face at each of the four, so two winners share no vertex, hence no face and no new
 *                   edge.  A winner writes its children into the parents' rows of faces_out and win[e] = 1;
 *   relax           one thread per vertex: row w of pos_out.  Class 0 with a one-ring of n > 0 moves, everything else is
 *                   copied.  q = (the sum of the ring in list order from its first entry) / n.  N is summed over the
 *                   edges (w, x) of w's list of sp_sd_hf_rm_vedge in order and, per edge, over its first and second face
 *                   in the order of their third vertices y: n = (p_x - p_w) x (p_y - p_w); the first n of finite
 *                   non-zero length is taken as it is, each later one is added when its dot product with that first one
 *                   is >= 0 and subtracted otherwise (the mesher's output is not consistently wound; nothing here
 *                   depends on the winding or on the order of the faces).  With nh = N / |N| (correctly rounded square
 *                   root and divisions) p' = q + ((p - q) . nh) nh; if |N| is 0 or not finite the vertex stays.
 * An index read from a table that is out of range makes its item a no-op (a status other than 0, "none", no winner, a
 * copy); nothing is addressed outside the buffers.  Host-side refusals (no launch): negative counts, NULL buffers, an
 * unknown mode, equal best buffers, low / high not positive and finite, a cosine outside [-1, 1].  Empty jobs return 0.
 * ---------------------------------------------------------------------------------- */
enum {
  NUDF_REMESH_CANDIDATE = 0,
  NUDF_REMESH_COUNT = 1,
  NUDF_REMESH_LONG = 2,
  NUDF_REMESH_CLASS = 3,
  NUDF_REMESH_BORDER = 4,
  NUDF_REMESH_LINK = 5,
  NUDF_REMESH_REACH = 6,
  NUDF_REMESH_FOLD = 7,
  NUDF_REMESH_DUPLICATE = 8,
  NUDF_REMESH_SAME = 9,
  NUDF_REMESH_EXISTS = 10,
  NUDF_REMESH_GAIN = 11
};
int nudf_meshremesh_collapse_check(const NudfMeshTopo* args, void* stream); /* one thread per unique edge */
int nudf_meshremesh_vertex_min(const NudfMeshTopo* args, void* stream);     /* one thread per vertex      */
int nudf_meshremesh_collapse_apply(const NudfMeshTopo* args, void* stream); /* one thread per unique edge */
int nudf_meshremesh_flip_check(const NudfMeshTopo* args, void* stream);     /* one thread per unique edge */
int nudf_meshremesh_flip_apply(const NudfMeshTopo* args, void* stream);     /* one thread per unique edge */
int nudf_meshremesh_relax(const NudfMeshTopo* args, void* stream);          /* one thread per vertex      */

/* ------------------------------------------------------------------------------------
 * Consistent face orientation and vertex normals (neuraludf_amd/meshclean.py orient_faces, vertex_normals): the step the
 * reference leaves out after its mesher because trimesh does it with a serial graph traversal ("DO NOT try to
 * consistently align winding directions: too slow and poor results", extract_mesh.py:218-219), and
 * trimesh.geometry.weighted_vertex_normals, which it calls at extract_mesh.py:272-275.  A struct of its own.
 * Half-edges and keys are NudfMeshTopo's.  A manifold edge is an undirected edge with exactly two
 * half-edges, of two different faces neither of which repeats a vertex; the caller lists them (me_a, me_b) from the sorted
 * keys.  Every face f holds one packed word, parent * 2 + parity, set to 2 f by the caller: parity = 1 says that f and its
 * parent need opposite flips.  One struct; each entry point reads the fields its comment names.
 *   hook     one thread per manifold edge: finds the roots of its two faces and the parities along the walks; the larger
 *            root takes 2 * the smaller + (pa ^ pb ^ [both half-edges start at the same vertex]) (64-bit atomicMin),
 *            *changed = 1;
 *   jump     one thread per face: word[f] = 2 * root + parity to the root (its own word only).  Rounds of hook + jump
 *            until *changed stays 0 end with word[f] >> 1 = the smallest face index of f's orientation component and, in
 *            an orientable component, word[f] & 1 = whether f is wound against that face;
 *   check    one thread per manifold edge, after the last round: nonorient[word[f] >> 1] = 1 where the parities of its
 *            two faces contradict the edge (the component is then not orientable);
 *   outward  one wavefront per component c: comp_sum[c] = sum over the faces comp_face[comp_off[c] .. comp_off[c + 1]) of
 *            N_f . (c_f - origin), N_f = (p1 - p0) x (p2 - p0) and c_f = (p0 + (p1 + p2)) / 3 with p1 and p2 swapped where
 *            word[f] & 1; lane l adds the faces l, l + 64, ... of the list in that order, then the 64 lane sums are added in
 *            lane order (float64, fixed order, no atomics);
 *   normals  one thread per vertex v: normals[v] = the normalised sum, over the corners corner[corner_off[v] ..
 *            corner_off[v + 1]) (corner 3 f + k, ascending), of atan2(|n_f|, e1 . e2) * n_f / |n_f|, n_f as N_f above without
 *            the swap, e1 / e2 the edges from the corner to the next / previous vertex of the face; a face with |n_f| = 0
 *            or not finite adds nothing; (0, 0, 0) where the sum has length 0 or is not finite.  float64.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfMeshOrient {
  const int64_t* faces;      /* [n_faces, 3]                                                                         */
  const int64_t* me_a;       /* [n_medges] first half-edge of each manifold edge (hook, check)                       */
  const int64_t* me_b;       /* [n_medges] its second half-edge (hook, check)                                        */
  int64_t* word;             /* [n_faces] parent * 2 + parity, set to 2 f by the caller (hook, jump; check, outward: read) */
  int32_t* changed;          /* one word, zeroed by the caller before each round (hook)                              */
  uint8_t* nonorient;        /* [n_faces] zeroed by the caller (check)                                               */
  const int64_t* comp_off;   /* [n_comps + 1] offsets into comp_face (outward)                                       */
  const int64_t* comp_face;  /* [n_faces] the faces grouped by component, ascending inside each (outward)            */
  double* comp_sum;          /* [n_comps] (outward)                                                                  */
  const double* pos;         /* [n_verts, 3] vertex positions (outward, normals)                                     */
  const int64_t* corner_off; /* [n_verts + 1] CSR offsets of the corners of each vertex (normals)                    */
  const int64_t* corner;     /* [3 n_faces] the corners 3 f + k, grouped by vertex, ascending inside each (normals)  */
  double* normals;           /* [n_verts, 3] (normals)                                                               */
  double origin[3];          /* outward: the point the faces should turn away from                                   */
  int64_t n_faces;
  int64_t n_verts;
  int64_t n_medges;
  int64_t n_comps;
  /* smoothing and denoising (appended, the version stays 111: see nudf_meshsmooth_* below)                           */
  const int64_t* sm_nbr_off; /* [n_verts + 1] CSR offsets of the one-ring of each vertex (laplace, uniform)          */
  const int64_t* sm_nbr;     /* [sm_n_nbr] the neighbours of each vertex, ascending (laplace, uniform)               */
  const uint8_t* sm_fixed;   /* NULL, or [n_verts]: non-zero = the vertex keeps its position (laplace, update)       */
  double* sm_pos_out;        /* [n_verts, 3] the positions after the step; must not alias pos (laplace, update)      */
  const double* sm_fnormal;  /* [n_faces, 3] unit face normals, (0, 0, 0) = the face takes no part (normals, update) */
  double* sm_fnormal_out;    /* [n_faces, 3] (frames, normals); must not alias sm_fnormal                            */
  double* sm_farea;          /* [n_faces] (frames: written; normals: read)                                           */
  double* sm_fcentre;        /* [n_faces, 3] (frames: written; normals: read)                                        */
  int64_t sm_n_nbr;          /* entries of sm_nbr                                                                    */
  double sm_step;            /* laplace: lambda or mu                                                                */
  double sm_inv2sc;          /* normals: 1 / (2 sigma_c^2), the spatial term                                         */
  double sm_inv2ss;          /* normals: 1 / (2 sigma_s^2), the normal term                                          */
  int32_t sm_weights;        /* laplace: 0 uniform, 1 cotangent                                                      */
  int32_t sm_pad_;
} NudfMeshOrient;
int nudf_meshorient_hook(const NudfMeshOrient* args, void* stream);        /* one thread per manifold edge    */
int nudf_meshorient_jump(const NudfMeshOrient* args, void* stream);        /* one thread per face             */
int nudf_meshorient_check(const NudfMeshOrient* args, void* stream);       /* one thread per manifold edge    */
int nudf_meshorient_outward(const NudfMeshOrient* args, void* stream);     /* one wavefront per component     */
int nudf_meshorient_normals(const NudfMeshOrient* args, void* stream);     /* one thread per vertex           */

/* ------------------------------------------------------------------------------------
 * Mesh smoothing and denoising (neuraludf_amd/meshclean.py smooth_mesh, denoise_mesh): Taubin's lambda | mu smoothing with
 * uniform or cotangent weights and the bilateral normal filter with a vertex update, the filters the reference's users
 * take to trimesh.smoothing or open3d on the CPU; the reference itself smooths border vertices only
 * (extract_mesh.py:238-265, nudf_meshtopo_smooth).  NudfMeshOrient grew at its end by the sm_ fields WITHOUT a version
 * step, as NudfPointCloud did for nudf_pc_raycast: the size table of nudf_abi_struct refuses a package and a library that
 * disagree.  faces, pos, corner_off, corner, n_faces and n_verts are those of nudf_meshorient_normals.  float64 without
 * contraction, every sum in list order inside one thread, no atomics; laplace, frames and update equal
 * tests/meshsmooth_ref.py bit for bit, normals up to the exp of its weight.  An index out of range
 * skips the corner, the neighbour or the face.
 *   laplace  one thread per vertex v: sm_pos_out[v] = pos[v] + sm_step (m - pos[v]).  sm_weights 0: m = the sum of pos[w]
 *            over sm_nbr[sm_nbr_off[v] .. sm_nbr_off[v + 1]) in list order, divided by their number.  1: over the corners
 *            of v in list order, corner (f, k) with a / b the next / previous vertex of f adds wa pos[a], then wb pos[b],
 *            wa = max(cot at b, 0) / 2, wb = max(cot at a, 0) / 2, the cot at c = (x - c) . (y - c) / |(x - c) x (y - c)|
 *            with x / y the next / previous vertex of c in f; a face in which one of the two lengths is 0 or not finite
 *            adds nothing; m = the sum / W, W = the sum of (wa + wb).  A vertex with sm_fixed[v] != 0, or whose W (or
 *            number of neighbours) is not finite or <= 0, copies its position;
 *   frames   one thread per face: with n = (p1 - p0) x (p2 - p0), sm_fnormal_out = n / |n|, (0, 0, 0) where |n| is 0 or
 *            not finite; sm_farea = |n| / 2; sm_fcentre = (p0 + (p1 + p2)) / 3.  All zero for a face with an index out of
 *            range;
 *   normals  one thread per face i: s = the sum of w n_j' over the faces j that share a vertex with i, met by walking the
 *            corner lists of i's vertices in ascending vertex index; j is skipped when j = i, when sm_fnormal[j] is
 *            (0, 0, 0) or when j holds a vertex of i walked earlier.  n_j' = n_j where n_i . n_j >= 0, else -n_j;
 *            w = sm_farea[j] exp(-(|c_i - c_j|^2 sm_inv2sc + |n_i - n_j'|^2 sm_inv2ss)).  sm_fnormal_out[i] = s / |s|, or
 *            n_i where |s| is 0 or not finite or n_i is (0, 0, 0);
 *   update   one thread per vertex v: sm_pos_out[v] = pos[v] + (the sum over the corners of v in list order of
 *            n_f (n_f . (c_f - pos[v]))) / count, n_f = sm_fnormal[f], c_f the centre of f from pos, count the corners
 *            with n_f != (0, 0, 0); a vertex with sm_fixed[v] != 0 or count = 0 copies its position.
 * Host-side refusals (no launch): n_verts >= 2^31, n_faces >= 2^36, a negative count, NULL buffers, sm_weights outside
 * {0, 1}, sm_step not finite, sm_inv2sc or sm_inv2ss not finite or <= 0.  Empty descriptors return 0.
 * ---------------------------------------------------------------------------------- */
int nudf_meshsmooth_laplace(const NudfMeshOrient* args, void* stream);     /* one thread per vertex           */
int nudf_meshsmooth_frames(const NudfMeshOrient* args, void* stream);      /* one thread per face             */
int nudf_meshsmooth_normals(const NudfMeshOrient* args, void* stream);     /* one thread per face             */
int nudf_meshsmooth_update(const NudfMeshOrient* args, void* stream);      /* one thread per vertex           */

/* ------------------------------------------------------------------------------------
 * Triangle rasteriser with a depth buffer (neuraludf_amd/meshrender.py rasterize, vertex_visibility, color_vertices): depth,
 * face and barycentric maps of a mesh from the dataset cameras, depth-tested vertex visibility and vertex colours blended
 * from the source images.  A struct of its own.  float64 without
 * contracted multiply-adds, integer atomics only: every result is identical from run to run.  A view is rows 0..2 of a world
 * matrix P, as `proj` of NudfMeshTopo; pixel (x, y) is the sample point with exactly those integer coordinates.  One struct;
 * each entry point reads the fields its comment names.  The caller passes `n_views` views at a time (a chunk of them, with
 * every per-view array pointing at the chunk's first view).
 *   project     one thread per (view, vertex): q = P p, each row as ((P0 x + P1 y) + P2 z) + P3;
 *               scr[view, v] = (q.x / q.z, q.y / q.z, q.z).  A vertex is valid in a view when all three are finite and
 *               q.z > 0;
 *   bounds      one thread per (view, face): npix[view, f] = (xmax - xmin + 1) (ymax - ymin + 1) with xmin = max(ceil(min x_i),
 *               0), xmax = min(floor(max x_i), W - 1), the same in y; 0 when a vertex index is out of range, the face repeats
 *               a vertex, a vertex is invalid in the view (no near-plane clipping), the signed area A = (x1 - x0)(y2 - y0) -
 *               (x2 - x0)(y1 - y0) is 0 or not finite, or the box is empty;
 *   draw_small  one thread per entry e of `entries` (view * n_faces + f, a (view, face) with npix > 0): every pixel (x, y) of
 *               the box, row-major.  The per-pixel function: w0 = (x1 - x)(y2 - y) - (x2 - x)(y1 - y), w1 = (x2 - x)(y0 - y) -
 *               (x0 - x)(y2 - y), w2 = (x0 - x)(y1 - y) - (x1 - x)(y0 - y); covered when all three are >= 0 or all three are
 *               <= 0 (two-sided, edges inclusive) and s = (w0 + w1) + w2 is finite and not 0; b_i = w_i / s; z = 1 / ((b0 / z0
 *               + b1 / z1) + b2 / z2); key = (uint64)bits(float32(z)) << 32 | f; zbuf[view, y, x] = min(zbuf, key) (64-bit
 *               unsigned atomicMin; the caller fills zbuf with all-ones).  Depth ties go to the smaller face index;
 *   draw_large  one wavefront per entry: lane l takes the pixels l, l + 64, ... of the box in row-major order, the same
 *               per-pixel function;
 *   resolve     one thread per pixel: all-ones -> depth +inf, face -1, bary (0, 0, 0); otherwise depth = the float32 of the
 *               key's high word, face = its low word, bary = float32(b_i) of the per-pixel function of that face at that
 *               pixel.  face and bary may be NULL (not written);
 *   visible     one thread per (view, vertex): vis[view, v] = 1 when the vertex is valid, (px, py) = round-half-even of
 *               scr.xy lies in [0, W - 1] x [0, H - 1], and float32(scr.z) <= m + min_gap (float32 sum), m = the maximum of
 *               depth[view] over [px - 1, px + 1] x [py - 1, py + 1] clamped to the image; else 0;
 *   colour      one thread per vertex, over the views in ascending order where vis[view, v] is set: (u, w, .) = the projection
 *               as in `project` (recomputed), x0 = floor(u), fx = u - x0, y0 = floor(w), fy = w - y0, taps at x0, x0 + 1 and
 *               y0, y0 + 1 clamped to the image, c = ((1 - fx)(1 - fy) c00 + fx (1 - fy) c10) + ((1 - fx) fy c01 + fx fy c11)
 *               per channel in float64, c10 the tap at x0 + 1 (uint8 taps are divided by 255 first); the weight g = 1 without
 *               normals, else pow(|n . d|, power), d = (cam_pos[view] - p) / |cam_pos[view] - p|, dot products and squared
 *               lengths summed as (x + y) + z; S = S + g, C = C + g c.  colors[v] = float32(C / S) and n_seen[v] = the number
 *               of such views; where S is not finite or not > 0, colors[v] = fill and n_seen[v] = 0.
 * ---------------------------------------------------------------------------------- */
typedef struct NudfMeshRaster {
  const double* pos;         /* [n_verts, 3] vertex positions (project, colour)                                      */
  const int64_t* faces;      /* [n_faces, 3] (bounds, draw_*, resolve)                                               */
  const double* proj;        /* [n_views, 3, 4] rows 0..2 of each world matrix (project, colour)                     */
  double* scr;               /* [n_views, n_verts, 3] (project: written; bounds, draw_*, resolve, visible: read)     */
  int32_t* npix;             /* [n_views, n_faces] (bounds)                                                          */
  const int64_t* entries;    /* [n_entries] view * n_faces + f, ascending (draw_*)                                   */
  uint64_t* zbuf;            /* [n_views, H, W] keys, all-ones = empty (draw_*: atomicMin; resolve: read)            */
  float* depth;              /* [n_views, H, W] (resolve: written; visible: read)                                    */
  int32_t* face;             /* [n_views, H, W] or NULL (resolve)                                                    */
  float* bary;               /* [n_views, H, W, 3] or NULL (resolve)                                                 */
  uint8_t* vis;              /* [n_views, n_verts] (visible: written; colour: read)                                  */
  const void* images;        /* [n_views, H, W, 3] uint8 or float32 (colour)                                         */
  const double* normals;     /* [n_verts, 3] unit vertex normals or NULL: weight 1 (colour)                          */
  const double* cam_pos;     /* [n_views, 3] camera centres, read with normals only (colour)                         */
  float* colors;             /* [n_verts, 3] (colour)                                                                */
  int32_t* n_seen;           /* [n_verts] (colour)                                                                   */
  int64_t n_faces;
  int64_t n_verts;
  int64_t n_entries;
  double power;              /* colour: exponent of |n . d|                                                          */
  float fill[3];             /* colour: the colour of a vertex no view contributes to                                */
  float min_gap;             /* visible: least camera-depth distance at which an occluder hides a vertex             */
  int32_t n_views;
  int32_t H;
  int32_t W;
  int32_t image_f32;         /* colour: 1 = float32 images, 0 = uint8                                                */
  /* texture atlases (nudf_meshtexture_*, below) */
  const double* tx_uv;       /* [n_faces, 3, 2] texel-centre coordinates of the corners of every face's chart       */
  const int64_t* tx_cell_face; /* [tx_n_cells, 2] the faces of the lower and the upper chart of a cell, -1 = none (bake) */
  const float* tx_fallback;  /* [n_verts, 3] colours mixed into texels no view contributes to, or NULL: fill (bake)  */
  float* tx_colors;          /* [tx_H, tx_W, 3] the texture (bake: written; shade: read)                             */
  int32_t* tx_n_seen;        /* [tx_H, tx_W] (bake)                                                                  */
  float* tx_out;             /* [n_views, H, W, 3] (shade)                                                           */
  int64_t tx_n_cells;
  int64_t tx_class_off[11];  /* Morton offset of every size class, and the end of the last, ascending (bake)         */
  int64_t tx_class_cell[11]; /* index of the first cell of every size class in tx_cell_face (bake)                   */
  int32_t tx_class_k[10];    /* log2 of the cell side of every size class, descending, each in [3, 12] (bake)        */
  int32_t tx_n_classes;      /* <= 10                                                                                */
  int32_t tx_W;              /* atlas width, a power of two                                                          */
  int32_t tx_H;              /* atlas height, tx_W or tx_W / 2                                                       */
  float tx_background[3];    /* shade: the colour of a pixel nothing was drawn into                                  */
} NudfMeshRaster;
int nudf_meshraster_project(const NudfMeshRaster* args, void* stream);     /* one thread per (view, vertex)   */
int nudf_meshraster_bounds(const NudfMeshRaster* args, void* stream);      /* one thread per (view, face)     */
int nudf_meshraster_draw_small(const NudfMeshRaster* args, void* stream);  /* one thread per entry            */
int nudf_meshraster_draw_large(const NudfMeshRaster* args, void* stream);  /* one wavefront per entry         */
int nudf_meshraster_resolve(const NudfMeshRaster* args, void* stream);     /* one thread per pixel            */
int nudf_meshraster_visible(const NudfMeshRaster* args, void* stream);     /* one thread per (view, vertex)   */
int nudf_meshraster_colour(const NudfMeshRaster* args, void* stream);      /* one thread per vertex           */

/* ------------------------------------------------------------------------------------
 * Texture atlases (neuraludf_amd/meshrender.py texture_atlas, bake_texture, shade_textured; csrc/meshtexture.hip): one
 * chart per face, a right isosceles triangle of texels, two charts to a square cell whose side s = 2^k is a power of two,
 * the cells packed by a prefix sum in Morton order; a bake that evaluates, per texel, what nudf_meshraster_colour evaluates
 * per vertex; and a textured draw of a raster.  NudfMeshRaster grew at its end by the tx_ fields WITHOUT a version step, as
 * NudfMeshOrient did for the sm_ fields: the size table of nudf_abi_struct refuses a package and a library that disagree.
 * Texel (i, j) of the atlas has its centre at (i, j): tx_uv is in those coordinates, and the texture is stored row-major,
 * texel (i, j) at [j, i].  float64 without contraction, no atomics, every sum inside one thread.
 * The layout (texture_atlas; torch on the device, restated by tests/meshtexture_ref.py):
 *   side     k_f = the smallest k in [3, 12] with 2^k - 6 >= L_f * density, 12 when there is none; L_f = the square root of
 *            the largest of the three squared edge lengths ((dx dx + dy dy) + dz dz, float64).  k_f = 3 for a face with a
 *            vertex index out of range, a repeated vertex or a squared edge length that is not finite;
 *   order    faces sorted by (k descending, face index ascending); the classes are the values of k that occur, descending;
 *            class c with n faces holds ceil(n / 2) cells, cell e of it the class's faces 2 e (lower chart) and 2 e + 1
 *            (upper chart, -1 when there is none); tx_class_cell[c] = the number of cells of the classes before c;
 *   place    tx_class_off[c] = the sum of cells 4^k over the classes before c, tx_class_off[n_classes] = the total T; cell e
 *            of class c covers the Morton indices [tx_class_off[c] + e 4^k, + 4^k): its corner (X, Y) is the even bits
 *            (X) and the odd bits (Y) of the first of them;
 *   size     tx_W = the smallest power of two with W^2 >= T (1 for T = 0), tx_H = W / 2 when 0 < T <= W^2 / 2, else W: the
 *            atlas is the Morton range [0, W H), the first half of a square's Morton range being its lower half;
 *   charts   in a cell of side s, local texel (i, j): the lower chart has its corners at (1, 1), (s - 4, 1), (1, s - 4), the
 *            upper one at (s - 2, s - 2), (4, s - 2), (s - 2, 4), both counter-clockwise; the lower face owns the texels
 *            with i + j <= s - 1, the upper face the others;
 *   corners  the face's corner opposite its longest edge (edge c joins the two corners other than c; squared lengths, the
 *            first maximum) sits at the right angle, the first corner listed above; the next two follow cyclically.
 *   bake     one thread per Morton index m of [0, tx_W tx_H): (i, j) = its even and odd bits.  c = the last class with
 *            tx_class_off[c] <= m; r = m - tx_class_off[c]; cell = tx_class_cell[c] + (r >> 2 k); the local (li, lj) = the
 *            even and odd bits of r mod 4^k; face = tx_cell_face[cell][li + lj <= s - 1 ? 0 : 1].  No owner (m >= T, cell >=
 *            tx_n_cells, face outside [0, n_faces)): tx_colors = fill, tx_n_seen = -1.  Otherwise, with (x_i, y_i) =
 *            tx_uv[face][i]: w0 = (x1 - i)(y2 - j) - (x2 - i)(y1 - j), w1 = (x2 - i)(y0 - j) - (x0 - i)(y2 - j), w2 =
 *            (x0 - i)(y1 - j) - (x1 - i)(y0 - j), b_i = w_i / ((w0 + w1) + w2), not clamped (the gutter extrapolates);
 *            p = (b0 p0 + b1 p1) + b2 p2 per coordinate.  Over the views in ascending order: s = the projection of p as in
 *            `project`; the view counts when s passes the test of `visible` (against depth[view], which holds every view);
 *            then the sample, the weight and the sums S, C of `colour`, the weight's normal being
 *            n = m t, m = (b0 n0 + b1 n1) + b2 n2 the mix of the corners' normals, t = l / |m| when |m| > 0, else 0,
 *            l = (b0 |n0| + b1 |n1|) + b2 |n2| (the mix rescaled to the length the corners' normals have: at a corner t is
 *            exactly 1 and the texel evaluates exactly the vertex).  tx_colors = float32(C / S), tx_n_seen = the number of
 *            such views; where S is not finite or not > 0, or the face has a vertex index out of range: tx_n_seen = 0 and
 *            tx_colors = fill, or with tx_fallback float32((b0 c0 + b1 c1) + b2 c2) of the corners' fallback colours in
 *            float64 (fill for a face with a vertex index out of range);
 *   shade    one thread per pixel of [n_views, H, W]: face[pixel] outside [0, n_faces) -> tx_out = tx_background; else
 *            (u, w) = (b0 uv0 + b1 uv1) + b2 uv2 with the float32 bary[pixel] taken in float64, and the bilinear sample of
 *            `colour` (x0 = floor(u), taps clamped to the atlas) of tx_colors, per channel, cast to float32.
 * Host-side refusals (no launch): the size checks of the rasteriser, tx_W or tx_H < 1, tx_W tx_H >= 2^31, tx_n_cells < 0,
 * tx_n_classes outside [0, 10], a tx_class_k outside [3, 12], tx_class_off or tx_class_cell not ascending from 0, NULL
 * buffers, a power that is not finite (bake, with normals).  Empty descriptors return 0 (bake: tx_W tx_H = 0; shade: no
 * pixels).
 * ---------------------------------------------------------------------------------- */
int nudf_meshtexture_bake(const NudfMeshRaster* args, void* stream);       /* one thread per Morton index     */
int nudf_meshtexture_shade(const NudfMeshRaster* args, void* stream);      /* one thread per pixel            */

#ifdef __cplusplus
}
#endif
#endif /* NUDF_H */
