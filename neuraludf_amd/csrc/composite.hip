// Fused UDF -> density -> alpha -> transmittance -> composite kernel (forward and backward).
//
// Replaces the ~90 elementwise torch ops, 2 cumprods and 9 reductions of
//   models/udf_renderer_blending.py:352-362 (dists / mid points), :370-423 (cosines, occlusion
//   probability, visibility scan, two-sided alphas), :484-553 (sphere masks, background concat,
//   transmittance scan, weighted sums, eikonal and sparsity sums), :151-159 (udf2logistic),
//   :292-320 (sdf2alpha 'numerical').
//
// One wavefront (64 lanes) per ray; sample i lives in lane i%64 of chunk i/64 (NC chunks in
// registers); both exclusive products are wave scans (shuffle based) with a carry across chunks.
// HBM-bound: 48 B/sample + 68 B/ray forward, 84 B/sample + 68 B/ray backward (algorithmic).
#include "nudf_common.h"
#include "../../include/nudf.h"
#include <stdlib.h>

// The kernel is VALU-bound with libm-accurate exp / divide / sqrt (~400 instructions per sample); the hardware
// transcendentals (v_exp_f32, v_rcp_f32, v_sqrt_f32: <= 1 ulp) cut that ~3x and make it HBM-bound.  Their error
// (1e-7 relative) is the same class as the fp32 rounding differences between two torch back ends.
#define CEXP(x) __expf(x)
#define CRCP(x) __builtin_amdgcn_rcpf(x)
#define CSQRT(x) __builtin_amdgcn_sqrtf(x)
__device__ __forceinline__ float csigmoid(float x) { return CRCP(1.0f + CEXP(-x)); }

struct PerSample {
  float z, dist, mid, u, gx, gy, gz, gm, tc, flip, raw, aocc, E_occ;
  float px, py, pz;
};

struct RayConst {
  float ox, oy, oz, dx, dy, dz;
  float inv_s, beta, gamma, sdist;
};

// inv_s, beta, gamma of a launch: from the clipped device vector, or formed here from the three parameters with
// scalars_fwd_kernel's expressions (rays_embed.hip; fields.py:654-655, 674-678 + the clips of :373-377)
__device__ __forceinline__ void comp_scalars(const NudfComposite& p, float& inv_s, float& beta, float& gamma) {
  if (p.p_variance) {
    inv_s = fminf(fmaxf(expf(10.0f * p.p_variance[0]), 1e-6f), 1e6f);
    beta = fminf(fmaxf(fminf(fmaxf(expf(10.0f * p.p_beta[0]), 0.0f), p.beta_hi), 1e-6f), 1e6f);
    gamma = fminf(fmaxf(expf(10.0f * p.p_gamma[0]), 1e-6f), 1e6f);
  } else {
    inv_s = p.scal[0]; beta = p.scal[1]; gamma = p.scal[2];
  }
}
__device__ __forceinline__ void comp_scalars_out(const NudfComposite& p, int32_t* status = nullptr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (p.p_variance) {
      float s, b, g;
      comp_scalars(p, s, b, g);
      if (p.scal_out) { p.scal_out[0] = s; p.scal_out[1] = b; p.scal_out[2] = g; }
      if (p.recip_out) { p.recip_out[0] = 1.0f / s; p.recip_out[1] = 1.0f / b; }
    }
    // the clips above are hardware min / max, which drop a NaN operand: a NaN parameter would otherwise train on
    // silently as inv_s = 1e-6 (torch's clip hands the NaN on, and the reference stops on it a few lines later)
    if (status) {
      const float chk = p.p_variance ? (p.p_variance[0] + p.p_beta[0]) + p.p_gamma[0] : (p.scal[0] + p.scal[1]) + p.scal[2];
      if (!(fabsf(chk) <= 3.0e38f)) atomicOr(status, NUDF_STATUS_NONFINITE_RENDER);
    }
  }
}

__device__ __forceinline__ float iter_cos_of(float c, int has_r, float r) {
  // c = -|true_cos| <= 0 ; udf_renderer_blending.py:295-299
  if (!has_r) return c;
  return -(fmaxf(-c * 0.5f + 0.5f, 0.0f) * (1.0f - r) + fmaxf(-c, 0.0f) * r);
}

struct AlphaOut {
  float a, P, Nx, num, den, ep, en;
};
__device__ __forceinline__ AlphaOut sdf2alpha_f(float sdf, float ic, float dist, float inv_s) {
  AlphaOut o;
  o.en = sdf + ic * dist * 0.5f;
  o.ep = sdf - ic * dist * 0.5f;
  o.P = csigmoid(o.ep * inv_s);
  o.Nx = csigmoid(o.en * inv_s);
  o.num = o.P - o.Nx + 1e-5f;
  o.den = o.P + 1e-5f;
  o.a = o.num * CRCP(o.den);
  return o;
}
// raw_occ = beta * l(beta u) with l(t) = e^-t / (1 + e^-t)^2 (udf2logistic, udf_renderer_blending.py:151-159): l and l' as
// autograd forms them from THAT expression, in e = e^-t -- l = e / (1 + e)^2, l' = l (e - 1) / (1 + e).  The sigmoid form
// sg (1 - sg) is the same function but cancels for t >> 1 (1 - sg is a multiple of 6e-8 where e ~ 1e-4).  Measured on the
// five full-size reference fixtures (round 6, gpurun_out/r6a): d loss / d beta 2.0e-3 ... 2.9e-3 TRUE relative away from
// the reference with the sigmoid form (the reference itself 0.4 ... 3e-4 from float64), 6e-6 ... 8e-5 with this one; the
// UDF weight gradients, which receive d udf from the same term, 7e-4 -> 9e-6.
__device__ __forceinline__ void logistic_pdf_terms(float beta, float u, float& ll, float& dl) {
  const float e = CEXP(-beta * u);
  const float r1e = CRCP(1.0f + e);
  ll = e * r1e * r1e;
  dl = ll * (e - 1.0f) * r1e;
}
__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// sdf2alpha before the clip, both variants (udf_renderer_blending.py:308-323): type 0 'numerical' (the shipped setting),
// type 1 'theorical' = 1 - exp(-relu(|iter_cos| inv_s (1 - sigmoid(sdf inv_s))) dist), which is in [0, 1) by itself
__device__ __forceinline__ float alpha_raw_f(int type, float sdf, float ic, float dist, float inv_s) {
  if (type == 0) return sdf2alpha_f(sdf, ic, dist, inv_s).a;
  const float raw = fabsf(ic) * inv_s * (1.0f - csigmoid(sdf * inv_s));
  return 1.0f - CEXP(-fmaxf(raw, 0.0f) * dist);
}
// adjoint of one side (sdf = sign * u) of the two-sided alpha: da -> d inv_s, d u, d iter_cos.  The caller has applied the
// clip's mask (0 <= alpha_raw <= 1).
__device__ __forceinline__ void alpha_bwd_f(int type, float sign, float u, float ic, float dist, float inv_s, float da,
                                            float& d_invs, float& du, float& dic) {
  if (type == 0) {
    AlphaOut o = sdf2alpha_f(sign * u, ic, dist, inv_s);
    const float rden = CRCP(o.den);
    const float dnum = da * rden;
    const float dden = -da * o.num * rden * rden;
    const float tP = (dnum + dden) * o.P * (1.0f - o.P);
    const float tN = (-dnum) * o.Nx * (1.0f - o.Nx);
    d_invs += tP * o.ep + tN * o.en;
    const float dep = tP * inv_s, den_ = tN * inv_s;
    du += sign * (dep + den_);
    dic += (den_ - dep) * dist * 0.5f;
    return;
  }
  const float sdf = sign * u;
  const float sg = csigmoid(sdf * inv_s), om = 1.0f - sg, aic = fabsf(ic);
  const float raw = aic * inv_s * om;
  const float draw = (raw > 0.0f) ? da * dist * CEXP(-raw * dist) : 0.0f;       // relu'(0) = 0 as in torch
  d_invs += draw * aic * om * (1.0f - inv_s * sg * sdf);
  du += sign * (-draw * aic * inv_s * inv_s * sg * om);
  dic += draw * inv_s * om * ((ic > 0.0f) ? 1.0f : ((ic < 0.0f) ? -1.0f : 0.0f));
}

// raw per-sample inputs.  ALL chunks of a ray are loaded before any arithmetic or store, so the HBM latency
// is paid once per ray instead of once per 64-sample chunk (stores to the diagnostic outputs would otherwise
// fence the next chunk's loads).
struct RawSample {
  float z, zn, u, gx, gy, gz;
};
// Row pointers of one ray.  The ray index is wave-uniform (made scalar with readfirstlane), so every address is
// <SGPR base> + <32-bit lane offset>: no 64-bit VALU address arithmetic (it was 9 % of the instructions).
struct RayRows {
  const float* z; const float* udf; const float* grad; const float* color; const float* color_base;
};
__device__ __forceinline__ RayRows ray_rows(const NudfComposite& p, int ray) {
  const size_t b = (size_t)ray * p.S;
  RayRows r;
  r.z = p.z + b; r.udf = p.udf + b; r.grad = p.grad + b * 3; r.color = p.color + b * 3; r.color_base = p.color_base + b * 3;
  return r;
}
__device__ __forceinline__ void load_raw(const RayRows& rr, int S, int i, RawSample& r) {
  // branch-free: the index is clamped into the ray (a divergent branch around a load makes the compiler wait
  // for all outstanding loads at the join); lanes past S load a valid duplicate that is never used
  // unsigned offsets: <SGPR base> + zero-extended 32-bit lane offset is the saddr addressing mode
  const unsigned ic = min((unsigned)i, (unsigned)(S - 1));
  r.z = rr.z[ic];
  r.zn = rr.z[min(ic + 1u, (unsigned)(S - 1))];
  r.u = rr.udf[ic];
  r.gx = rr.grad[ic * 3u + 0u];
  r.gy = rr.grad[ic * 3u + 1u];
  r.gz = rr.grad[ic * 3u + 2u];
}

// shared per-sample evaluation (phase A)
__device__ __forceinline__ void eval_sample(const NudfComposite& p, const RayConst& rc, int i, const RawSample& r,
                                            PerSample& s) {
  const int S = p.S;
  s.z = r.z;
  s.dist = (i < S - 1) ? (r.zn - s.z) : rc.sdist;
  s.mid = s.z + s.dist * 0.5f;
  s.px = rc.ox + rc.dx * s.mid;
  s.py = rc.oy + rc.dy * s.mid;
  s.pz = rc.oz + rc.dz * s.mid;
  s.u = r.u;
  s.gx = r.gx;
  s.gy = r.gy;
  s.gz = r.gz;
  s.gm = CSQRT(s.gx * s.gx + s.gy * s.gy + s.gz * s.gz);
  const float rgme = CRCP(s.gm + 1e-5f);  // gradients / (|g| + 1e-5)  (:370-371)
  const float cn = rc.dx * (s.gx * rgme) + rc.dy * (s.gy * rgme) + rc.dz * (s.gz * rgme);
  s.tc = p.use_norm_grad ? cn : (rc.dx * s.gx + rc.dy * s.gy + rc.dz * s.gz);
  s.flip = (cn > 0.0f) ? -1.0f : 1.0f;  // -sign(cos), 0 -> 1  (:386-388)
  const float e = CEXP(-rc.beta * s.u);
  const float r1e = CRCP(1.0f + e);
  s.raw = rc.beta * e * r1e * r1e;  // udf2logistic(udf, beta, 1, 1)
  s.E_occ = CEXP(-fmaxf(s.raw, 0.0f) * rc.gamma * s.dist);
  s.aocc = 1.0f - s.E_occ;
}

// FULL: S == 64 * NC, no outside samples, s_nominal >= S -- every lane of every chunk holds a live inside sample, so
// none of the liveness selects / compares exist in that instantiation (cfg 2 and cfg 5 shapes).
// Iteration schedules from device memory (NudfComposite.sched): the two by-value scalars that change from iteration to
// iteration -- cos_anneal_ratio and flip_saturation -- are then read here, so a captured HIP graph of the train step
// (kernel arguments frozen at capture) follows the schedules.  Uniform scalar loads, once per kernel.
#define NUDF_COMPOSITE_SCHED(p)                \
  if ((p).sched) {                             \
    (p).cos_anneal = (p).sched[0];             \
    (p).flip_saturation = (p).sched[1];        \
  }

template <int NC, bool DIAG, bool FULL>
__global__ __launch_bounds__(256) void composite_fwd_kernel(NudfComposite p, int32_t* status) {
  NUDF_COMPOSITE_SCHED(p)
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int ray = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  __shared__ float red[4][5];
  float s_relax_n = 0.f, s_relax_d = 0.f, s_near_n = 0.f, s_near_d = 0.f, s_sparse = 0.f;

  if (ray < p.N) {
    const int S = p.S, NO = p.n_out, ST = S + NO;
    RayConst rc;
    rc.ox = p.rays_o[ray * 3 + 0]; rc.oy = p.rays_o[ray * 3 + 1]; rc.oz = p.rays_o[ray * 3 + 2];
    rc.dx = p.rays_d[ray * 3 + 0]; rc.dy = p.rays_d[ray * 3 + 1]; rc.dz = p.rays_d[ray * 3 + 2];
    comp_scalars(p, rc.inv_s, rc.beta, rc.gamma); rc.sdist = p.sample_dist[0];

    float tcv[NC], aocc[NC], alpha[NC], apv[NC], amv[NC], flipv[NC], midv[NC];
    float cr[NC], cg[NC], cb[NC], br[NC], bg[NC], bb[NC], nx[NC], ny[NC], nz[NC];

    // ---- phase 0: every load of this ray, branch-free --------------------------------------
    RawSample raw[NC];
    float bgz[NC], bgzn[NC], bgs[NC];
    const RayRows rr = ray_rows(p, ray);
    const bool has_col = p.color != nullptr;
    float* __restrict__ wrow = p.weights + (size_t)ray * ST;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      load_raw(rr, S, i, raw[c]);
      const unsigned b = min((unsigned)i, (unsigned)(S - 1));
      if (has_col) {   // (uniform; weights-first launches leave the colour sums to the colour network's epilogue)
        cr[c] = rr.color[b * 3u + 0u]; cg[c] = rr.color[b * 3u + 1u]; cb[c] = rr.color[b * 3u + 2u];
        br[c] = rr.color_base[b * 3u + 0u]; bg[c] = rr.color_base[b * 3u + 1u]; bb[c] = rr.color_base[b * 3u + 2u];
      } else {
        cr[c] = cg[c] = cb[c] = br[c] = bg[c] = bb[c] = 0.f;
      }
      bgz[c] = bgzn[c] = bgs[c] = 0.f;
    }
    if (!FULL && NO > 0) {  // uniform
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int i = c * 64 + l;
        if ((c + 1) * 64 <= S) continue;  // uniform: this chunk holds no outside sample
        const unsigned j = (unsigned)min(max(i - S, 0), NO - 1);
        const float* bz = p.bg_z + (size_t)ray * NO;
        const float* bs = p.bg_sigma + (size_t)ray * NO;
        const float* bc = p.bg_color + (size_t)ray * NO * 3;
        bgz[c] = bz[j];
        bgzn[c] = bz[min(j + 1u, (unsigned)(NO - 1))];
        bgs[c] = bs[j];
        const float q0 = bc[j * 3u + 0u], q1 = bc[j * 3u + 1u], q2 = bc[j * 3u + 2u];
        const bool out = i >= S;
        cr[c] = out ? q0 : cr[c]; cg[c] = out ? q1 : cg[c]; cb[c] = out ? q2 : cb[c];
        br[c] = out ? q0 : br[c]; bg[c] = out ? q1 : bg[c]; bb[c] = out ? q2 : bb[c];
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bool live = FULL || (c * 64 + l) < ST;
      cr[c] = live ? cr[c] : 0.f; cg[c] = live ? cg[c] : 0.f; cb[c] = live ? cb[c] : 0.f;
      br[c] = live ? br[c] : 0.f; bg[c] = live ? bg[c] : 0.f; bb[c] = live ? bb[c] : 0.f;
    }

    // ---- phase A: per-sample quantities --------------------------------------------------
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      tcv[c] = 0.f; aocc[c] = 0.f; alpha[c] = 0.f; apv[c] = 0.f; amv[c] = 0.f; flipv[c] = 1.f; midv[c] = 0.f;
      nx[c] = ny[c] = nz[c] = 0.f;
      if (FULL || i < S) {
        PerSample s;
        eval_sample(p, rc, i, raw[c], s);
        tcv[c] = s.tc; aocc[c] = s.aocc; flipv[c] = s.flip; midv[c] = s.mid;
        nx[c] = s.flip * s.gx; ny[c] = s.flip * s.gy; nz[c] = s.flip * s.gz;
        const size_t b = (size_t)ray * S + i;
        // sdf2alpha(+-udf, -|true_cos|, dist, inv_s, cos_anneal_ratio)  (:414-417)
        const float ic = iter_cos_of(-fabsf(s.tc), p.has_anneal, p.cos_anneal);
        apv[c] = clip01(alpha_raw_f(p.alpha_type, s.u, ic, s.dist, rc.inv_s));
        amv[c] = clip01(alpha_raw_f(p.alpha_type, -s.u, ic, s.dist, rc.inv_s));
        // eikonal / sparsity partial sums (:484-487, 531-536, 553)
        const float pn = CSQRT(s.px * s.px + s.py * s.py + s.pz * s.pz);
        const float ge = (s.gm - 1.0f) * (s.gm - 1.0f);
        if (pn < 1.2f) { s_relax_n += ge; s_relax_d += 1.0f; }
        if (s.u < 0.05f) { s_near_n += ge; s_near_d += 1.0f; }
        s_sparse += CEXP(-p.sparse_scale * s.u);
        if (DIAG) {
          if (p.o_alpha_occ) p.o_alpha_occ[b] = s.aocc;
          if (p.o_raw_occ) p.o_raw_occ[b] = s.raw;
          if (p.o_true_cos) p.o_true_cos[b] = s.tc;
          if (p.o_grad_mag) p.o_grad_mag[b] = s.gm;
          if (p.o_mid_z) p.o_mid_z[b] = s.mid;
          if (p.o_dists) p.o_dists[b] = s.dist;
          if (p.o_inside) p.o_inside[b] = (pn < 1.0f) ? 1.0f : 0.0f;
          if (p.o_flip) p.o_flip[b] = s.flip;
        }
      } else if (!FULL && i < ST) {
        const float dist = (i < ST - 1) ? (bgzn[c] - bgz[c]) : rc.sdist;
        alpha[c] = 1.0f - CEXP(-fmaxf(bgs[c], 0.0f) * dist);  // :181
      }
    }

    // ---- phase B: visibility probability = exclusive product scan (:400-412) ------------
    // the NC per-chunk scans are independent (the carry multiplies afterwards): interleaved DPP steps
    float carry = 1.0f;
    float qs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      // vis_mask shifted by one sample: mask_i = (true_cos_{i+1} < 0.01), last = 1
      const float tn_other = (c + 1 < NC) ? wave_bcast(tcv[(c + 1 < NC) ? c + 1 : c], 0) : 0.f;
      const float tnext = wave_shift_down1(tcv[c], tn_other);
      float vm = (i < S - 1) ? ((tnext < 0.01f) ? 1.0f : 0.0f) : 1.0f;
      qs[c] = (FULL || i < S) ? (clip01(1.0f - aocc[c] + p.flip_saturation * vm) + 1e-7f) : 1.0f;
    }
    wave_incl_scan_mul_n<NC>(qs);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      const float inc = qs[c] * carry;
      const float exc = wave_shift_up1(inc, carry);
      carry = wave_bcast(inc, 63);
      if (FULL || i < S) {
        const float vis = clip01(exc);
        alpha[c] = apv[c] * vis + amv[c] * (1.0f - vis);
        if (DIAG) {
          const size_t b = (size_t)ray * S + i;
          if (p.o_vis_prob) p.o_vis_prob[b] = vis;
          if (p.o_alpha) p.o_alpha[b] = alpha[c];
          if (p.o_alpha_plus) p.o_alpha_plus[b] = apv[c];
          if (p.o_alpha_minus) p.o_alpha_minus[b] = amv[c];
        }
      }
    }

    // ---- phase C: transmittance scan + weighted sums (:508-526, 568) --------------------
    carry = 1.0f;
    float a_cr = 0, a_cg = 0, a_cb = 0, a_br = 0, a_bg = 0, a_bb = 0, a_depth = 0, a_nx = 0, a_ny = 0, a_nz = 0;
    float a_ws = 0, a_wall = 0;
    float fs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) fs[c] = (FULL || (c * 64 + l) < ST) ? (1.0f - alpha[c] + 1e-7f) : 1.0f;
    wave_incl_scan_mul_n<NC>(fs);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      const float inc = fs[c] * carry;
      const float exc = wave_shift_up1(inc, carry);
      carry = wave_bcast(inc, 63);
      const float w = (FULL || i < ST) ? alpha[c] * exc : 0.0f;
      if (FULL || i < ST) wrow[i] = w;
      a_cr += w * cr[c]; a_cg += w * cg[c]; a_cb += w * cb[c];
      a_br += w * br[c]; a_bg += w * bg[c]; a_bb += w * bb[c];
      a_wall += w;
      if (FULL || i < p.s_nominal) a_ws += w;
      if (FULL || i < S) {
        a_depth += w * midv[c];
        a_nx += w * nx[c]; a_ny += w * ny[c]; a_nz += w * nz[c];
      }
    }
    {
      float r[12] = {a_cr, a_cg, a_cb, a_br, a_bg, a_bb, a_depth, a_nx, a_ny, a_nz, a_ws, a_wall};
      wave_sum_n<12>(r);
      a_cr = r[0]; a_cg = r[1]; a_cb = r[2]; a_br = r[3]; a_bg = r[4]; a_bb = r[5];
      a_depth = r[6]; a_nx = r[7]; a_ny = r[8]; a_nz = r[9]; a_ws = r[10]; a_wall = r[11];
    }
    if (l == 0) {
      float bgr = 0.f, bgg = 0.f, bgb = 0.f;
      if (p.background_rgb) {  // colour += background_rgb * (1 - weights_sum)  (:527-528)
        bgr = p.background_rgb[0] * (1.0f - a_wall);
        bgg = p.background_rgb[1] * (1.0f - a_wall);
        bgb = p.background_rgb[2] * (1.0f - a_wall);
      }
      if (has_col) {
        p.out_color[ray * 3 + 0] = a_cr + bgr; p.out_color[ray * 3 + 1] = a_cg + bgg; p.out_color[ray * 3 + 2] = a_cb + bgb;
        p.out_color_base[ray * 3 + 0] = a_br; p.out_color_base[ray * 3 + 1] = a_bg; p.out_color_base[ray * 3 + 2] = a_bb;
      }
      p.out_depth[ray] = a_depth;
      p.out_normals[ray * 3 + 0] = a_nx; p.out_normals[ray * 3 + 1] = a_ny; p.out_normals[ray * 3 + 2] = a_nz;
      p.out_wsum[ray] = a_ws;
      p.out_wsum_all[ray] = a_wall;
      // a non-finite composited output of the ray (the values are in registers: seven additions and one compare per ray;
      // the atomic only fires when something is wrong -- nudf_set_status_flag)
      if (status && !(fabsf(((a_wall + a_depth) + (a_cr + a_cg)) + ((a_cb + a_br) + (a_bg + a_bb))) <= 3.0e38f))
        atomicOr(status, NUDF_STATUS_NONFINITE_RENDER);
    }
  }

  // ---- batch-global sums: wave -> block -> one atomic per block ---------------------------
  {
    float r[5] = {s_relax_n, s_relax_d, s_near_n, s_near_d, s_sparse};
    wave_sum_n<5>(r);
    if (l == 0) {
      red[wave][0] = r[0]; red[wave][1] = r[1]; red[wave][2] = r[2]; red[wave][3] = r[3]; red[wave][4] = r[4];
    }
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    float t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (p.ws) p.ws[(size_t)blockIdx.x * 5 + threadIdx.x] = t;   // summed by partial_sums_kernel
    else atomicAdd(p.sums + threadIdx.x, t);
  }  comp_scalars_out(p, status);
}

// out[k] = sum_b ws[b * K + k]  (one block of 1024 threads; fixed order -> deterministic batch-global sums; ASSIGNS).
// Thread t owns the block rows t, t + 1024, ... and keeps all K (<= 8) running sums, so the partials are read once,
// coalesced; then one DPP wave reduction per k and a 16-entry LDS pass.  (The first version reduced one k at a time
// with an LDS tree per k: 27 us for 8192 blocks, a quarter of the whole composite forward at 32768 rays.)
// the second stage's arithmetic (1024 threads): thread t owns rows t, t + 1024, ...; one wave reduction per k; 16 wave
// results added in order.  res[k] valid in threads < K after the call.
__device__ __forceinline__ float partial_sums_body(const float* __restrict__ ws, int nblk, int K, float (&red)[8][16]) {
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 1024) {
    const float* row = ws + (size_t)b * K;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < K) acc[k] += row[k];
  }
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < K) {
      const float t = wave_sum(acc[k]);
      if (l == 0) red[k][wave] = t;
    }
  }
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < K)
    for (int w = 0; w < 16; ++w) t += red[threadIdx.x][w];
  return t;
}

// partial_sums + scalars_bwd_kernel (rays_embed.hip) as one launch: d inv_s / d beta / d gamma summed over the blocks, then
// through the exp and the clips to the three parameters
__global__ __launch_bounds__(1024) void partial_sums_scalars_kernel(const float* __restrict__ ws, int nblk,
                                                                    const float* variance, const float* beta,
                                                                    const float* gamma, float beta_hi,
                                                                    float* __restrict__ d_scal_out,
                                                                    float* __restrict__ d_param) {
  __shared__ float red[8][16];
  __shared__ float ds[3];
  const float t = partial_sums_body(ws, nblk, 3, red);
  if (threadIdx.x < 3) {
    ds[threadIdx.x] = t;
    if (d_scal_out) d_scal_out[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = expf(10.0f * variance[0]);
    d_param[0] = (s >= 1e-6f && s <= 1e6f) ? ds[0] * 10.0f * s : 0.0f;
    const float b = expf(10.0f * beta[0]);
    const float b1 = fminf(fmaxf(b, 0.0f), beta_hi);
    d_param[1] = (b >= 0.0f && b <= beta_hi && b1 >= 1e-6f && b1 <= 1e6f) ? ds[1] * 10.0f * b : 0.0f;
    const float g = expf(10.0f * gamma[0]);
    d_param[2] = (g >= 1e-6f && g <= 1e6f) ? ds[2] * 10.0f * g : 0.0f;
  }
}

__global__ __launch_bounds__(1024) void partial_sums_kernel(const float* __restrict__ ws, int nblk, int K,
                                                            float* __restrict__ out) {
  __shared__ float red[8][16];
  const float t = partial_sums_body(ws, nblk, K, red);
  if (threadIdx.x < K) out[threadIdx.x] = t;
}

// ------------------------------------------------------------------------------------------
// backward: recompute the forward per ray, then two reverse (suffix) scans
// ------------------------------------------------------------------------------------------
template <int NC, bool FULL>
__global__ __launch_bounds__(256) void composite_bwd_kernel(NudfComposite p, NudfCompositeGrad g) {
  NUDF_COMPOSITE_SCHED(p)
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int ray = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  __shared__ float red[4][3];
  float d_invs = 0.f, d_beta = 0.f, d_gamma = 0.f;

  if (ray < p.N) {
    const int S = p.S, NO = p.n_out, ST = S + NO;
    RayConst rc;
    rc.ox = p.rays_o[ray * 3 + 0]; rc.oy = p.rays_o[ray * 3 + 1]; rc.oz = p.rays_o[ray * 3 + 2];
    rc.dx = p.rays_d[ray * 3 + 0]; rc.dy = p.rays_d[ray * 3 + 1]; rc.dz = p.rays_d[ray * 3 + 2];
    comp_scalars(p, rc.inv_s, rc.beta, rc.gamma); rc.sdist = p.sample_dist[0];

    // upstream gradients (per ray)
    const float dCr = g.d_color ? g.d_color[ray * 3 + 0] : 0.f, dCg = g.d_color ? g.d_color[ray * 3 + 1] : 0.f,
                dCb = g.d_color ? g.d_color[ray * 3 + 2] : 0.f;
    const float dBr = g.d_color_base ? g.d_color_base[ray * 3 + 0] : 0.f,
                dBg = g.d_color_base ? g.d_color_base[ray * 3 + 1] : 0.f,
                dBb = g.d_color_base ? g.d_color_base[ray * 3 + 2] : 0.f;
    const float dDepth = g.d_depth ? g.d_depth[ray] : 0.f;
    const float dNx = g.d_normals ? g.d_normals[ray * 3 + 0] : 0.f, dNy = g.d_normals ? g.d_normals[ray * 3 + 1] : 0.f,
                dNz = g.d_normals ? g.d_normals[ray * 3 + 2] : 0.f;
    const float dWs = g.d_wsum ? g.d_wsum[ray] : 0.f;
    float dWall = g.d_wsum_all ? g.d_wsum_all[ray] : 0.f;
    if (p.background_rgb && g.d_color)
      dWall -= dCr * p.background_rgb[0] + dCg * p.background_rgb[1] + dCb * p.background_rgb[2];
    const float k_relax = g.d_sums ? g.d_sums[0] : 0.f, k_near = g.d_sums ? g.d_sums[2] : 0.f,
                k_sparse = g.d_sums ? g.d_sums[4] : 0.f;

    PerSample ps[NC];
    float q[NC], inner[NC], Vraw[NC], vis[NC], ap_raw[NC], am_raw[NC], alpha[NC], T[NC], w[NC], f[NC], dw[NC], icv[NC];
    float bg_dist[NC], bg_E[NC];

    // ---- phase 0: every load of this ray, branch-free (see load_raw) ------------------------------
    RawSample raw[NC];
    float cdot[NC], dwup[NC], bgz[NC], bgzn[NC], bgs[NC];
    const RayRows rr = ray_rows(p, ray);
    const float* dwrow = g.d_weights ? g.d_weights + (size_t)ray * ST : nullptr;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      load_raw(rr, S, i, raw[c]);
      const unsigned b = min((unsigned)i, (unsigned)(S - 1));
      // the colours only enter the backward through <upstream, colour>
      cdot[c] = dCr * rr.color[b * 3u + 0u] + dCg * rr.color[b * 3u + 1u] + dCb * rr.color[b * 3u + 2u] +
                dBr * rr.color_base[b * 3u + 0u] + dBg * rr.color_base[b * 3u + 1u] + dBb * rr.color_base[b * 3u + 2u];
      dwup[c] = dwrow ? dwrow[min((unsigned)i, (unsigned)(ST - 1))] : 0.f;
      bgz[c] = bgzn[c] = bgs[c] = 0.f;
    }
    if (!FULL && NO > 0) {  // uniform
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int i = c * 64 + l;
        if ((c + 1) * 64 <= S) continue;  // uniform
        const int j = min(max(i - S, 0), NO - 1);
        const size_t b = (size_t)ray * NO + j;
        bgz[c] = p.bg_z[b];
        bgzn[c] = p.bg_z[b + ((j < NO - 1) ? 1 : 0)];
        bgs[c] = p.bg_sigma[b];
        const float q = (dCr + dBr) * p.bg_color[b * 3 + 0] + (dCg + dBg) * p.bg_color[b * 3 + 1] +
                        (dCb + dBb) * p.bg_color[b * 3 + 2];
        cdot[c] = (i >= S) ? q : cdot[c];
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bool live = FULL || (c * 64 + l) < ST;
      cdot[c] = live ? cdot[c] : 0.f;
      dwup[c] = live ? dwup[c] : 0.f;
    }

    // ---- recompute phase A ------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      ps[c].tc = 0.f; ps[c].aocc = 0.f; alpha[c] = 0.f; bg_dist[c] = 0.f; bg_E[c] = 1.f; icv[c] = 0.f;
      ap_raw[c] = am_raw[c] = 0.f;
      if (FULL || i < S) {
        eval_sample(p, rc, i, raw[c], ps[c]);
        icv[c] = iter_cos_of(-fabsf(ps[c].tc), p.has_anneal, p.cos_anneal);
      } else if (!FULL && i < ST) {
        bg_dist[c] = (i < ST - 1) ? (bgzn[c] - bgz[c]) : rc.sdist;
        bg_E[c] = CEXP(-fmaxf(bgs[c], 0.0f) * bg_dist[c]);
        alpha[c] = 1.0f - bg_E[c];
      }
    }
    // ---- recompute phase B ------------------------------------------------------------------
    float carry = 1.0f;
    float sc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      const float tn_other = (c + 1 < NC) ? wave_bcast(ps[(c + 1 < NC) ? c + 1 : c].tc, 0) : 0.f;
      const float tnext = wave_shift_down1(ps[c].tc, tn_other);
      float vm = (i < S - 1) ? ((tnext < 0.01f) ? 1.0f : 0.0f) : 1.0f;
      inner[c] = 1.0f - ps[c].aocc + p.flip_saturation * vm;
      q[c] = (FULL || i < S) ? (clip01(inner[c]) + 1e-7f) : 1.0f;
      sc[c] = q[c];
    }
    wave_incl_scan_mul_n<NC>(sc);       // the per-chunk scans are independent: interleaved DPP steps
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      const float inc = sc[c] * carry;
      const float exc = wave_shift_up1(inc, carry);
      carry = wave_bcast(inc, 63);
      Vraw[c] = exc;
      vis[c] = clip01(exc);
      if (FULL || i < S) {
        ap_raw[c] = alpha_raw_f(p.alpha_type, ps[c].u, icv[c], ps[c].dist, rc.inv_s);
        am_raw[c] = alpha_raw_f(p.alpha_type, -ps[c].u, icv[c], ps[c].dist, rc.inv_s);
        alpha[c] = clip01(ap_raw[c]) * vis[c] + clip01(am_raw[c]) * (1.0f - vis[c]);
      }
    }
    // ---- recompute phase C + upstream d w ---------------------------------------------------
    carry = 1.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      f[c] = (FULL || (c * 64 + l) < ST) ? (1.0f - alpha[c] + 1e-7f) : 1.0f;
      sc[c] = f[c];
    }
    wave_incl_scan_mul_n<NC>(sc);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      const float inc = sc[c] * carry;
      const float exc = wave_shift_up1(inc, carry);
      carry = wave_bcast(inc, 63);
      T[c] = exc;
      w[c] = (FULL || i < ST) ? alpha[c] * exc : 0.0f;
      float d = 0.f;
      if (FULL || i < ST) {
        d = dWall + dwup[c] + cdot[c];
        if (FULL || i < p.s_nominal) d += dWs;
      }
      if (FULL || i < S) {
        const unsigned b = (unsigned)i;
        d += dDepth * ps[c].mid + ps[c].flip * (dNx * ps[c].gx + dNy * ps[c].gy + dNz * ps[c].gz);
        // colours receive w * upstream
        if (g.o_d_color) {
          float* o = g.o_d_color + (size_t)ray * S * 3;
          o[b * 3u + 0u] = w[c] * dCr; o[b * 3u + 1u] = w[c] * dCg; o[b * 3u + 2u] = w[c] * dCb;
        }
        if (g.o_d_color_base) {
          float* o = g.o_d_color_base + (size_t)ray * S * 3;
          o[b * 3u + 0u] = w[c] * dBr; o[b * 3u + 1u] = w[c] * dBg; o[b * 3u + 2u] = w[c] * dBb;
        }
      } else if (!FULL && i < ST) {
        const size_t b = (size_t)ray * NO + (i - S);
        if (g.o_d_bg_color) {
          g.o_d_bg_color[b * 3 + 0] = w[c] * (dCr + dBr); g.o_d_bg_color[b * 3 + 1] = w[c] * (dCg + dBg);
          g.o_d_bg_color[b * 3 + 2] = w[c] * (dCb + dBb);
        }
      }
      dw[c] = d;
    }

    // ---- reverse scan 1: d alpha through the transmittance product -------------------------
    //   d f_i = (sum_{j>i} dw_j w_j) / f_i ;  d alpha_i = dw_i T_i - d f_i
    float dalpha[NC];
    float rcarry = 0.0f;
    float rs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) rs[c] = dw[c] * w[c];
    wave_incl_rscan_add_n<NC>(rs);
#pragma unroll
    for (int c = NC - 1; c >= 0; --c) {
      const float v = dw[c] * w[c];
      float incl = rs[c] + rcarry;  // sum_{j>=i}
      float excl = incl - v;                          // sum_{j>i}
      rcarry = wave_bcast(incl, 0);
      dalpha[c] = dw[c] * T[c] - excl * CRCP(f[c]);
    }

    // ---- local backward to vis / alpha+- ; reverse scan 2 through the visibility product ---
    float dV_V[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = c * 64 + l;
      dV_V[c] = 0.f;
      if (FULL || i < S) {
        const float dvis = dalpha[c] * (clip01(ap_raw[c]) - clip01(am_raw[c]));
        const float dV = (Vraw[c] >= 0.0f && Vraw[c] <= 1.0f) ? dvis : 0.0f;
        dV_V[c] = dV * Vraw[c];
      } else if (!FULL && i < ST) {
        // background alpha = 1 - exp(-relu(sigma) dist)
        const size_t b = (size_t)ray * NO + (i - S);
        if (g.o_d_bg_sigma) g.o_d_bg_sigma[b] = (bgs[c] > 0.0f) ? dalpha[c] * bg_E[c] * bg_dist[c] : 0.0f;
      }
    }
    rcarry = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) rs[c] = dV_V[c];
    wave_incl_rscan_add_n<NC>(rs);
#pragma unroll
    for (int c = NC - 1; c >= 0; --c) {
      const int i = c * 64 + l;
      const float v = dV_V[c];
      float incl = rs[c] + rcarry;
      float excl = incl - v;
      rcarry = wave_bcast(incl, 0);
      if (FULL || i < S) {
        const PerSample& s = ps[c];
        const float dq = excl * CRCP(q[c]);
        const float daocc = (inner[c] >= 0.0f && inner[c] <= 1.0f) ? -dq : 0.0f;
        // alpha_occ = 1 - exp(-relu(raw) gamma dist)
        const float rr = fmaxf(s.raw, 0.0f);
        const float draw = (s.raw > 0.0f) ? daocc * s.E_occ * rc.gamma * s.dist : 0.0f;
        d_gamma += daocc * s.E_occ * rr * s.dist;
        // raw = beta * sg (1 - sg), sg = sigmoid(beta u)
        float ll, dl;
        logistic_pdf_terms(rc.beta, s.u, ll, dl);
        float du = draw * rc.beta * rc.beta * dl;
        d_beta += draw * (ll + rc.beta * s.u * dl);

        // two-sided alphas
        float dic = 0.f;
        const float dap = dalpha[c] * vis[c], dam = dalpha[c] * (1.0f - vis[c]);
#pragma unroll
        for (int sgn = 0; sgn < 2; ++sgn) {
          const float sign = sgn ? -1.0f : 1.0f;
          const float a_raw = sgn ? am_raw[c] : ap_raw[c];
          const float da = sgn ? dam : dap;
          if (a_raw >= 0.0f && a_raw <= 1.0f) alpha_bwd_f(p.alpha_type, sign, s.u, icv[c], s.dist, rc.inv_s, da, d_invs, du, dic);
        }
        // iter_cos -> c = -|tc| -> tc
        const float cc = -fabsf(s.tc);
        float dic_dc = 1.0f;
        if (p.has_anneal) dic_dc = 0.5f * (1.0f - p.cos_anneal) + ((cc < 0.0f) ? p.cos_anneal : 0.0f);
        const float sgn_tc = (s.tc > 0.0f) ? 1.0f : ((s.tc < 0.0f) ? -1.0f : 0.0f);
        const float dtc = dic * dic_dc * (-sgn_tc);

        // gradient-vector adjoint
        float dgx, dgy, dgz;
        if (p.use_norm_grad) {
          const float rg = CRCP(s.gm + 1e-5f);
          const float dotg = dtc * (rc.dx * s.gx + rc.dy * s.gy + rc.dz * s.gz);
          const float k2 = (s.gm > 0.0f) ? dotg * CRCP(s.gm) * rg * rg : 0.0f;
          dgx = dtc * rc.dx * rg - s.gx * k2;
          dgy = dtc * rc.dy * rg - s.gy * k2;
          dgz = dtc * rc.dz * rg - s.gz * k2;
        } else {
          dgx = dtc * rc.dx; dgy = dtc * rc.dy; dgz = dtc * rc.dz;
        }
        // normals = sum w * flip * g
        dgx += w[c] * s.flip * dNx; dgy += w[c] * s.flip * dNy; dgz += w[c] * s.flip * dNz;
        // eikonal sums
        const float pn = CSQRT(s.px * s.px + s.py * s.py + s.pz * s.pz);
        float dgm = 0.f;
        if (pn < 1.2f) dgm += k_relax * 2.0f * (s.gm - 1.0f);
        if (s.u < 0.05f) dgm += k_near * 2.0f * (s.gm - 1.0f);
        if (s.gm > 0.0f) {
          const float t = dgm * CRCP(s.gm);
          dgx += t * s.gx; dgy += t * s.gy; dgz += t * s.gz;
        }
        // sparsity sum
        du += k_sparse * (-p.sparse_scale) * CEXP(-p.sparse_scale * s.u);

        float* ou = g.o_d_udf + (size_t)ray * S;
        float* og = g.o_d_grad + (size_t)ray * S * 3;
        const unsigned b = (unsigned)i;
        ou[b] = du;
        og[b * 3u + 0u] = dgx; og[b * 3u + 1u] = dgy; og[b * 3u + 2u] = dgz;
      }
    }
  }

  {
    float r[3] = {d_invs, d_beta, d_gamma};
    wave_sum_n<3>(r);
    if (l == 0) { red[wave][0] = r[0]; red[wave][1] = r[1]; red[wave][2] = r[2]; }
  }
  __syncthreads();
  if (threadIdx.x < 3 && (g.o_d_scal || g.ws)) {
    float t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (g.ws) g.ws[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
    else atomicAdd(g.o_d_scal + threadIdx.x, t);
  }
}

#define NUDF_MAX_CHUNKS 8
// chunks of the instantiation that serves nc chunks of samples: <1> ... <6> are compiled, nc = 7 and 8 share <8>
static inline int composite_chunks(int nc) { return nc <= 6 ? nc : NUDF_MAX_CHUNKS; }

extern "C" int nudf_composite_fwd(const NudfComposite* args, void* stream) {
  const NudfComposite& p = *args;
  if (p.N <= 0) return 0;
  const int ST = p.S + p.n_out;
  const int nc = (ST + 63) / 64;
  if (nc > NUDF_MAX_CHUNKS || p.S < 1) {
    nudf_set_error("nudf_composite_fwd: 1 <= S, S + n_outside <= 512 required", hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  if ((p.color == nullptr) != (p.color_base == nullptr) || (!p.color && (p.n_out > 0 || p.bg_color))) {
    nudf_set_error("nudf_composite_fwd: color and color_base are given together; the weights-first form (both NULL) has no "
                   "outside samples", hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  if ((p.defer_sums && !p.ws) || (p.p_variance && (!p.p_beta || !p.p_gamma)) || (!p.p_variance && !p.scal)) {
    nudf_set_error("nudf_composite_fwd: defer_sums needs ws; scalars need scal or all three parameters", hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  dim3 grid((p.N + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  int32_t* status = nudf_status_flag();
  // diagnostics (the 12 per-sample arrays of the full result dict) are a separate instantiation: the training path
  // carries no stores, branches or address arithmetic for them
  const bool diag = p.o_alpha_occ || p.o_raw_occ || p.o_true_cos || p.o_grad_mag || p.o_mid_z || p.o_dists ||
                    p.o_inside || p.o_flip || p.o_vis_prob || p.o_alpha || p.o_alpha_plus || p.o_alpha_minus;
  // FULL promises a live sample in every lane of every INSTANTIATED chunk: nc = 7 runs <8> with a dead chunk, so
  // S = 448 is not FULL (it used to be: the dead chunk's lanes then stored 64 weights past the ray's row)
  const bool full = (p.S == 64 * composite_chunks(nc)) && p.n_out == 0 && p.s_nominal >= p.S;
#define NUDF_CF_LAUNCH(NCV)                                                                                   \
  if (diag) hipLaunchKernelGGL((composite_fwd_kernel<NCV, true, false>), grid, block, 0, st, p, status);      \
  else if (full) hipLaunchKernelGGL((composite_fwd_kernel<NCV, false, true>), grid, block, 0, st, p, status); \
  else hipLaunchKernelGGL((composite_fwd_kernel<NCV, false, false>), grid, block, 0, st, p, status)
  switch (nc) {
    case 1: NUDF_CF_LAUNCH(1); break;
    case 2: NUDF_CF_LAUNCH(2); break;
    case 3: NUDF_CF_LAUNCH(3); break;
    case 4: NUDF_CF_LAUNCH(4); break;
    case 5: NUDF_CF_LAUNCH(5); break;
    case 6: NUDF_CF_LAUNCH(6); break;
    default: NUDF_CF_LAUNCH(8); break;
  }
#undef NUDF_CF_LAUNCH
  if (p.ws && !p.defer_sums) hipLaunchKernelGGL(partial_sums_kernel, dim3(1), dim3(1024), 0, st, p.ws, (int)grid.x, 5, p.sums);
  NUDF_CHECK_LAUNCH("nudf_composite_fwd");
  return 0;
}

// second stage of the backward's d inv_s / d beta / d gamma: plain sums into o_d_scal, or (o_d_param) the sums taken on
// through scalars_bwd's expressions to the three parameters in the same launch
static void composite_bwd_reduce(const NudfComposite& p, const NudfCompositeGrad& g, int nblk, hipStream_t st) {
  if (!g.ws) return;
  if (g.o_d_param && p.p_variance)
    hipLaunchKernelGGL(partial_sums_scalars_kernel, dim3(1), dim3(1024), 0, st, g.ws, nblk, p.p_variance, p.p_beta, p.p_gamma,
                       p.beta_hi, g.o_d_scal, g.o_d_param);
  else if (g.o_d_scal)
    hipLaunchKernelGGL(partial_sums_kernel, dim3(1), dim3(1024), 0, st, g.ws, nblk, 3, g.o_d_scal);
}

extern "C" int nudf_composite_bwd(const NudfComposite* args, const NudfCompositeGrad* grads, void* stream) {
  const NudfComposite& p = *args;
  if (p.N <= 0) return 0;
  const int ST = p.S + p.n_out;
  const int nc = (ST + 63) / 64;
  if (nc > NUDF_MAX_CHUNKS || p.S < 1) {
    nudf_set_error("nudf_composite_bwd: 1 <= S, S + n_outside <= 512 required", hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  dim3 grid((p.N + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  const bool full = (p.S == 64 * composite_chunks(nc)) && p.n_out == 0 && p.s_nominal >= p.S;   // (see nudf_composite_fwd)
#define NUDF_CB_LAUNCH(NCV)                                                                         \
  if (full) hipLaunchKernelGGL((composite_bwd_kernel<NCV, true>), grid, block, 0, st, p, *grads);   \
  else hipLaunchKernelGGL((composite_bwd_kernel<NCV, false>), grid, block, 0, st, p, *grads)
  switch (nc) {
    case 1: NUDF_CB_LAUNCH(1); break;
    case 2: NUDF_CB_LAUNCH(2); break;
    case 3: NUDF_CB_LAUNCH(3); break;
    case 4: NUDF_CB_LAUNCH(4); break;
    case 5: NUDF_CB_LAUNCH(5); break;
    case 6: NUDF_CB_LAUNCH(6); break;
    default: NUDF_CB_LAUNCH(8); break;
  }
#undef NUDF_CB_LAUNCH
  composite_bwd_reduce(p, *grads, (int)grid.x, st);
  NUDF_CHECK_LAUNCH("nudf_composite_bwd");
  return 0;
}

// per-ray colours from the 32-point partial sums the colour chain's SIGMOIDN epilogues left (NudfChainStep.row_sums)
__global__ void colour_finish_kernel(const float* __restrict__ sc, const float* __restrict__ sb, int N, int nb,
                                     const float* __restrict__ background_rgb, const float* __restrict__ wsum_all,
                                     float* __restrict__ out_c, float* __restrict__ out_b) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * 3) return;
  const int ray = idx / 3, c = idx - ray * 3;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < nb; ++k) {
    a += sc[((size_t)ray * nb + k) * 4 + c];
    if (sb) b += sb[((size_t)ray * nb + k) * 4 + c];
  }
  if (background_rgb) a += background_rgb[c] * (1.0f - wsum_all[ray]);
  out_c[idx] = a;
  if (out_b) out_b[idx] = b;
}
extern "C" int nudf_composite_colour_finish(const float* sums_color, const float* sums_color_base, int N, int S,
                                            const float* background_rgb, const float* wsum_all, float* out_color,
                                            float* out_color_base, void* stream) {
  if (N <= 0) return 0;
  if (S < 32 || (S & 31) || !sums_color || !out_color || (background_rgb && !wsum_all) || (!sums_color_base != !out_color_base)) {
    nudf_set_error("nudf_composite_colour_finish: S a positive multiple of 32 (rays = whole 32-point blocks) required",
                   hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(colour_finish_kernel, dim3((N * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums_color,
                     sums_color_base, N, S / 32, background_rgb, wsum_all, out_color, out_color_base);
  NUDF_CHECK_LAUNCH("nudf_composite_colour_finish");
  return 0;
}

extern "C" int nudf_partial_sums(const float* ws, int nblk, int K, float* out, void* stream) {
  if (nblk < 0 || K < 1 || K > 8) {
    nudf_set_error("nudf_partial_sums: 1 <= K <= 8 required", hipErrorInvalidValue);
    return (int)hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(partial_sums_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ws, nblk, K, out);
  NUDF_CHECK_LAUNCH("nudf_partial_sums");
  return 0;
}
