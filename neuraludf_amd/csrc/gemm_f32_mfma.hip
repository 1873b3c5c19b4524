// fp32 MFMA GEMMs for the MLP chains of the NeuralUDF hot path (gfx950).
//
//   gemm_nn : C[M,N]   = epilogue( A[M,K] * B[K,N] )         A,B row-major, K % 32 == 0
//   (the weight-gradient contraction gemm_tn lives in gemm_tn_f32_mfma.hip)
//
// v_mfma_f32_32x32x2_f32 (exact fp32, == an fmaf chain), 64x64x32 block tiles, 4 waves (2x2), each wave one
// 32x32 MFMA tile, single LDS buffer + register prefetch.
// These replace the chains of F.linear / weight_norm / Softplus / ReLU / autograd ops of
// models/fields.py:192-231 (UDFNetwork), :452-495 (ResidualRenderingNetwork), :599-628 (NeRF)
// and their (double-)backward.  MFMA peak for this instruction: 157.3 TFLOP/s.
#include "nudf_common.h"
#include "../../include/nudf.h"

#define BM 64
#define BN 64
#define BK 32
#define LDA_S (BM + 1)  // As[k][m]: +1 pad makes the transposing ds_write_b32 conflict-free
#define LDB_S (BN + 4)  // Bs[k][n]: rows stay 16-byte aligned for ds_write_b128
#define A_TILE (BK * LDA_S)
#define B_TILE (BK * LDB_S)

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int xcd_swizzle(int b, int nblk) {
  // blocks are dealt round-robin to the 8 XCDs; make consecutive logical tiles (which share
  // an A row-tile) land on the same XCD's L2.  Speed only.
  return ((nblk & 7) == 0) ? (b & 7) * (nblk >> 3) + (b >> 3) : b;
}

// softplus'(a) = s and 1 - s recovered from the STORED activation h = softplus100(a) * (1/xscale):
//   1 - s = exp(-100 h), s = -expm1(-100 h)  (exact identities; no 1 - s cancellation near s = 1, which
//   matters for softplus'' = 100 s (1 - s) in the second-order backward).  Above torch's threshold
//   (100 a > 20 <=> h > 0.2) autograd uses s = 1, s' = 0.
__device__ __forceinline__ void sp_derivs_from_h(float hstored, float xscale, float& s, float& om) {
  const float x = 100.0f * xscale * hstored;
  if (x > 20.0f) {
    s = 1.0f;
    om = 0.0f;
  } else {
    const float e = __expf(-x);
    om = e;
    s = (x < 0.01f) ? x * (1.0f - x * (0.5f - x * 0.16666667f)) : 1.0f - e;
  }
}

template <int EPI>
__device__ __forceinline__ void epilogue_store(const NudfGemmNN& p, int row, int col, float acc) {
  float v = acc;
  if (p.bias) v += p.bias[col];
  const size_t r = (size_t)row;
  if (EPI == NUDF_EPI_NONE) {
    p.C1[r * p.ldc1 + col] = v * p.scale;
  } else if (EPI == NUDF_EPI_SOFTPLUS) {
    // nn.Softplus(beta=100, threshold=20) and its derivative from ONE hardware exp (v_exp_f32):
    //   z = e^{100 v}; h = log1p(z)/100; h' = z/(1+z)   (above the threshold: h = v, h' = 1)
    // log1pf, not log(1 + z): for 1e-4 <= z <= 1e-2 the sum 1 + z has already dropped the bits of z that h consists of
    // (measured: 5.4e-4 of h over that window, profiles/r10_layer_matrix.txt; 5.9e-4 at z = 1e-4 itself with exact exp / log,
    // tests/test_layer_ref.py), and the stored h is what the backward recovers h' from.
    const float t = 100.0f * v;
    float h = v;
    if (t <= 20.0f) h = log1pf(__expf(t)) * 0.01f;
    p.C1[r * p.ldc1 + col] = h * p.scale;
    if (p.C2) p.C2[r * p.ldc2 + col] = (t <= 20.0f) ? __fdividef(__expf(t), 1.0f + __expf(t)) : 1.0f;
  } else if (EPI == NUDF_EPI_RELU) {
    p.C1[r * p.ldc1 + col] = fmaxf(v, 0.0f) * p.scale;
  } else if (EPI == NUDF_EPI_MUL) {
    p.C1[r * p.ldc1 + col] = v * p.X1[r * p.ldx1 + col] * p.scale;
  } else if (EPI == NUDF_EPI_MULMASK) {
    p.C1[r * p.ldc1 + col] = (p.X1[r * p.ldx1 + col] > 0.0f) ? v * p.scale : 0.0f;
  } else if (EPI == NUDF_EPI_MULSP) {
    float sg, om;
    sp_derivs_from_h(p.X1[r * p.ldx1 + col], p.xscale, sg, om);
    p.C1[r * p.ldc1 + col] = v * sg * p.scale;
  } else if (EPI == NUDF_EPI_TANGENT) {
    float sg, om;
    sp_derivs_from_h(p.X1[r * p.ldx1 + col], p.xscale, sg, om);
    p.C1[r * p.ldc1 + col] = v * sg * p.scale;
    // X2 = da = delta * s, so  acc * delta * softplus''  =  acc * da * 100 (1 - s)
    p.C2[r * p.ldc2 + col] = v * p.X2[r * p.ldx2 + col] * 100.0f * om;
  } else if (EPI == NUDF_EPI_BWD) {
    float sg, om;
    sp_derivs_from_h(p.X1[r * p.ldx1 + col], p.xscale, sg, om);
    p.C1[r * p.ldc1 + col] = v * p.scale * sg + (p.X2 ? p.X2[r * p.ldx2 + col] : 0.0f);
  } else if (EPI == NUDF_EPI_SIGMOID) {
    // first iparam columns through a sigmoid (optionally mirrored into C2), the rest raw
    if (col < p.iparam) {
      float s = sigmoidf_(v);
      p.C1[r * p.ldc1 + col] = s;
      if (p.C2) p.C2[r * p.ldc2 + col] = s;
    } else if (p.C3) {
      p.C3[r * p.ldc3 + (col - p.iparam)] = v;
    } else {
      p.C1[r * p.ldc1 + col] = v;
    }
  } else if (EPI == NUDF_EPI_UDFHEAD) {
    // channel 0 = |x| * scale (the 'abs' UDF head, fields.py:184-190, 210) -> C2[row], its sign ->
    // C3[row] (kept for the backward); channels 1.. (the appearance feature) -> C1[row, col-1]
    if (col == 0) {
      // udf_out and its derivative by p.iparam: 0 'abs', 1 'square', 2 'sdf' (fields.py:184-190)
      const float hv = (p.iparam == 1) ? v * v : ((p.iparam == 2) ? v : fabsf(v));
      const float hm = (p.iparam == 1) ? 2.0f * v : ((p.iparam == 2) ? 1.0f : ((v > 0.0f) ? 1.0f : ((v < 0.0f) ? -1.0f : 0.0f)));
      if (p.C2) p.C2[r] = hv * p.scale;
      if (p.C3) p.C3[r] = hm;
    } else if (p.C1) {
      p.C1[r * p.ldc1 + (col - 1)] = v;
    }
  } else if (EPI == NUDF_EPI_SKIPSPLIT) {
    // reverse sweep through the skip concat: columns < iparam belong to the hidden branch
    // (times softplus' and scale), the rest go to the embedding branch (times scale)
    if (col < p.iparam) {
      float sg, om;
      sp_derivs_from_h(p.X1[r * p.ldx1 + col], p.xscale, sg, om);
      p.C1[r * p.ldc1 + col] = v * sg * p.scale;
    } else {
      p.C2[r * p.ldc2 + (col - p.iparam)] = v * p.scale;
    }
  } else if (EPI == NUDF_EPI_RELU_DUAL) {
    // relu output to two destinations (hidden tap of the colour net, fields.py:472-473)
    float h = fmaxf(v, 0.0f);
    p.C1[r * p.ldc1 + col] = h;
    if (p.C2) p.C2[r * p.ldc2 + col] = h;
  } else if (EPI == NUDF_EPI_ADDMASK) {
    p.C1[r * p.ldc1 + col] = (p.X1[r * p.ldx1 + col] > 0.0f) ? (v + p.X2[r * p.ldx2 + col]) * p.scale : 0.0f;
  }
}

// ---------------------------------------------------------------------------------------
// C[M,N] = epilogue(A[M,K] B[K,N]).  Block = 4 waves (2x2); each wave owns one 32x32 MFMA tile of the 64x64 block
// tile.  One LDS buffer (17 KB) + register prefetch, two barriers per k-step; many small co-resident blocks, whose epilogues
// (HBM-bound) overlap the other blocks' MFMA phases.
// Measured on MI355X (profiles/r01_gemm_variants.txt): the 64x64 tile wins on every shape of this workload over
// 128x128 (single / double-buffered) and 64x128 -- these layer GEMMs sit at the fp32 ridge (K = 128..256, several
// [M,N] epilogue operands), so overlapping many small blocks matters more than LDS reuse.  Those variants are retired.
// ---------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256, 6) void gemm_nn_kernel(NudfGemmNN p) {
  constexpr int APASS = BM / 32, BPASS = BN / 32;  // float4 loads per thread per k-step
  __shared__ __attribute__((aligned(16))) float smem[A_TILE + B_TILE];
  float* As = smem;
  float* Bs = smem + A_TILE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int lb = xcd_swizzle(blockIdx.x, gridDim.x);
  const int m0 = (lb / tiles_n) * BM;
  const int n0 = (lb % tiles_n) * BN;
  const int nk = p.K / BK;

  int a_off[APASS], b_off[BPASS];
  int a_lds[APASS], b_lds[BPASS];
  bool b_ok[BPASS];
#pragma unroll
  for (int ps = 0; ps < APASS; ++ps) {
    const int idx = ps * 256 + tid;
    const int row = idx >> 3, kq = idx & 7;
    int gr = m0 + row;
    if (gr > p.M - 1) gr = p.M - 1;
    a_off[ps] = gr * p.lda + kq * 4;
    a_lds[ps] = (kq * 4) * LDA_S + row;
  }
#pragma unroll
  for (int ps = 0; ps < BPASS; ++ps) {
    const int idx = ps * 256 + tid;
    const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
    const int gc = n0 + c4 * 4;
    b_ok[ps] = gc < p.ldb;
    b_off[ps] = kr * p.ldb + (b_ok[ps] ? gc : 0);
    b_lds[ps] = kr * LDB_S + c4 * 4;
  }

  f32x4 ra[APASS], rb[BPASS];
  auto gload = [&](int kt) {
    const float* Ak = p.A + kt * BK;
    const float* Bk = p.B + (size_t)kt * BK * p.ldb;
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) ra[ps] = *reinterpret_cast<const f32x4*>(Ak + a_off[ps]);
#pragma unroll
    for (int ps = 0; ps < BPASS; ++ps)
      rb[ps] = b_ok[ps] ? *reinterpret_cast<const f32x4*>(Bk + b_off[ps]) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto sstore = [&]() {
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
      float* d = As + a_lds[ps];
      d[0] = ra[ps].x;
      d[LDA_S] = ra[ps].y;
      d[2 * LDA_S] = ra[ps].z;
      d[3 * LDA_S] = ra[ps].w;
    }
#pragma unroll
    for (int ps = 0; ps < BPASS; ++ps) *reinterpret_cast<f32x4*>(Bs + b_lds[ps]) = rb[ps];
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  // wave-uniform: live column tiles of this wave, 0 or 1 (N may end inside the block tile)
  const int ncol_act = min(1, max(0, (p.N - (n0 + wn * 32) + 31) / 32));

  auto compute = [&]() {
    const float* as = As + (lane >> 5) * LDA_S + wm * 32 + (lane & 31);
    const float* bs = Bs + (lane >> 5) * LDB_S + wn * 32 + (lane & 31);
    // (a loop over 0 or 1 tiles, not an `if`: hipcc orders the kernel's address arithmetic differently for the `if`, and these
    // 13 kernels stay instruction for instruction the ones that were measured)
    for (int j = 0; j < ncol_act; ++j) {
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) acc = mfma32(as[(2 * kk) * LDA_S], bs[(2 * kk) * LDB_S], acc);
    }
  };

  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    sstore();
    __syncthreads();
    if (kt + 1 < nk) gload(kt + 1);
    compute();
    __syncthreads();
  }

  if (ncol_act == 0) return;
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= p.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < p.M) epilogue_store<EPI>(p, row, col, acc[r]);
  }
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
template <int EPI>
static int launch_nn(const NudfGemmNN& p, hipStream_t st) {
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  hipLaunchKernelGGL((gemm_nn_kernel<EPI>), dim3(tiles), dim3(256), 0, st, p);
  NUDF_CHECK_LAUNCH("nudf_gemm_nn");
  return 0;
}

extern "C" int nudf_gemm_nn(const NudfGemmNN* args, void* stream) {
  const NudfGemmNN& p = *args;
  hipStream_t st = (hipStream_t)stream;
  if (p.M <= 0 || p.N <= 0) return 0;
  if (p.K <= 0 || (p.K % BK) != 0 || (p.lda % 4) != 0 || (p.ldb % 4) != 0 ||
      (((uintptr_t)p.A) & 15) || (((uintptr_t)p.B) & 15)) {
    nudf_set_error("nudf_gemm_nn: K%32, lda%4, ldb%4 and 16-byte alignment required", hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  switch (p.epi) {
    case NUDF_EPI_NONE: return launch_nn<NUDF_EPI_NONE>(p, st);
    case NUDF_EPI_SOFTPLUS: return launch_nn<NUDF_EPI_SOFTPLUS>(p, st);
    case NUDF_EPI_RELU: return launch_nn<NUDF_EPI_RELU>(p, st);
    case NUDF_EPI_MUL: return launch_nn<NUDF_EPI_MUL>(p, st);
    case NUDF_EPI_MULMASK: return launch_nn<NUDF_EPI_MULMASK>(p, st);
    case NUDF_EPI_TANGENT: return launch_nn<NUDF_EPI_TANGENT>(p, st);
    case NUDF_EPI_BWD: return launch_nn<NUDF_EPI_BWD>(p, st);
    case NUDF_EPI_SIGMOID: return launch_nn<NUDF_EPI_SIGMOID>(p, st);
    case NUDF_EPI_UDFHEAD: return launch_nn<NUDF_EPI_UDFHEAD>(p, st);
    case NUDF_EPI_SKIPSPLIT: return launch_nn<NUDF_EPI_SKIPSPLIT>(p, st);
    case NUDF_EPI_RELU_DUAL: return launch_nn<NUDF_EPI_RELU_DUAL>(p, st);
    case NUDF_EPI_ADDMASK: return launch_nn<NUDF_EPI_ADDMASK>(p, st);
    case NUDF_EPI_MULSP: return launch_nn<NUDF_EPI_MULSP>(p, st);
    default:
      nudf_set_error("nudf_gemm_nn: unknown epilogue", hipErrorInvalidValue);
      return (int)hipErrorInvalidValue;
  }
}
