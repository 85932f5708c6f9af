// Losses for class-imbalanced tasks as the fourth stage of a level's loss chain: Tversky and focal Tversky terms (Salehi et al.;
// Abraham & Khan) per class, per sample or over the batch (nnU-Net's batch_dice), and a focal cross-entropy on the label's channel
// (gamma_f = 0: the plain mean cross-entropy).  2 <= C <= 8.  With t_c = [label == c] (0 in every class where label >= C) the sums
// pass accumulates, per (sample, class) and each directly,
//     I = sum p t     FP = sum p (1 - t)     FN = sum t (1 - p)     F = sum t (1 - p)^gf (-log max(p, 1e-6))
// FP and FN are never formed as P - I and T - I: with p[label] == 1.0 on most voxels that subtraction cancels and can come out
// negative, which a fractional power of 1 - TI does not survive.  The class weight a_c of the focal term does not depend on the
// voxel and multiplies F in the finalize kernel.
//     Tversky term of class c:  1 - TI = (alpha FP + beta FN) / (I + alpha FP + beta FN + eps)
//         per sample: value = (1 / B) sum_b (1 - TI[b])^(1 / gamma);  batch: I, FP, FN summed over b first, value = (1 - TI)^(1 / gamma)
//     focal cross-entropy:      value = (1 / (B S)) sum_{b, c} a_c F[b, c]
//     total = base + scale (sum_k w_k value_k + w_focal value_focal)
// and every gradient has the form  dp[b, s, c] = gscale (A[b, c] + t (Bc[b, c] + G[b, c] f'(p))),  f = (1 - p)^gf log max(p, 1e-6),
// with coef [B][C][3] = (A, Bc, G) written by the finalize kernel, already weighted and scaled: one streaming pass, as loss.hip.
// Where 1 - TI is exactly 0 and gamma > 1 the power's derivative is infinite; the term's gradient there is 0 (the chosen
// subgradient).  f' is that of the clamped expression: below p = 1e-6 the (1 - p)^gf / p part is absent.
// Built on loss_stream.h: per-workgroup partials folded in a fixed order, no floating-point atomics, no host read.
#include "loss_stream.h"

#include <math.h>

#define IMB_MAX_K 8

struct ImbCfg {
  int K;                          // Tversky terms
  int cls[IMB_MAX_K];             // class of term k
  float w[IMB_MAX_K];             // weight of term k
  float alpha, beta, inv_gamma, eps;
  int batch;                      // I, FP, FN summed over the batch before the ratio
  float w_focal;
  float a[LTU_WIDE_MAXC];         // class weights of the focal term
};

// how the focal factor (1 - p)^gf is formed: 0: gf == 0 (the factor is 1), 1: gf == 1, 2: gf == 2, 3: any other gf in [1, 5];
// a negative gf (the sums pass of a call whose w_focal is 0) is mode -1: no log, no F
__device__ __forceinline__ int imb_mode(float gf) { return gf < 0.f ? -1 : gf == 0.f ? 0 : gf == 1.f ? 1 : gf == 2.f ? 2 : 3; }

// q^(gf - 1) for q = 1 - p >= 0, gf >= 1: exact for gf = 1 and 2; q = 0 gives 0 for gf > 1 (exp2(-inf))
__device__ __forceinline__ float imb_pow1(float q, float gf, int mode) {
  return mode == 1 ? 1.f : mode == 2 ? q : exp2f((gf - 1.f) * log2f(q));
}

// One voxel into {I, FP, FN, F} of each class.  The rounding is written out as in loss.hip: p t and p (1 - t) are exact, t (1 - p)
// is one rounded difference, and the focal factor meets the F sum in one fused multiply-add with the log, whatever the class count.
template <int C>
__device__ __forceinline__ void imb_add(int lab, const float* f, float gf, int mode, float (&acc)[C * 4]) {
  float pl = 1.f;
#pragma unroll
  for (int c = 0; c < C; ++c) pl = lab == c ? f[c] : pl;
  const float q = fmaxf(1.f - pl, 0.f);
  const float pw = mode < 0 ? 0.f : mode == 0 ? 1.f : ls_rounded(q * imb_pow1(q, gf, mode));
  const float nl = mode < 0 ? 0.f : 0.f - logf(fmaxf(pl, 1e-6f));
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float pc = f[c];
    const bool t = lab == c;
    acc[c * 4 + 0] += t ? pc : 0.f;
    acc[c * 4 + 1] += t ? 0.f : pc;
    acc[c * 4 + 2] += t ? 1.f - pc : 0.f;
    acc[c * 4 + 3] = fmaf(t ? pw : 0.f, nl, acc[c * 4 + 3]);
  }
}

// p f32 [B][S][C], label u8 [B][S]; sums [1 + block][B][C][4] = {I, FP, FN, F}.  V4: four voxels per thread and trip, two trips in
// flight up to C = 4 (loss_stream.h)
template <int C, bool V4>
__global__ void __launch_bounds__(256) imb_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ sums,
                                                       long long S, int rows_per_block, float gf) {
  float acc[C * 4];
#pragma unroll
  for (int k = 0; k < C * 4; ++k) acc[k] = 0.f;
  const int mode = imb_mode(gf);
  ls_walk_block<C, V4, (C <= 4)>(p, label, S, rows_per_block, [&](int lab, const float* f) { imb_add<C>(lab, f, gf, mode, acc); });
  ls_store_partial<C * 4>(acc, sums);
}

// v = (1 - TI)^(1 / gamma) of one (I, FP, FN), and its derivative as the two coefficients of a voxel: dv/dp = a + t bc
__device__ __forceinline__ void imb_tversky(float I, float FP, float FN, const ImbCfg& cfg, float& v, float& a, float& bc) {
  const float num = fmaf(cfg.alpha, FP, ls_rounded(cfg.beta * FN));
  const float ie = I + cfg.eps;
  const float den = ie + num;
  const float r = num / den;                      // 1 - TI, in [0, 1)
  float dv;                                       // dv/dr
  if (cfg.inv_gamma == 1.f) { v = r; dv = 1.f; }
  else if (r > 0.f) { v = powf(r, cfg.inv_gamma); dv = cfg.inv_gamma * v / r; }
  else { v = 0.f; dv = 0.f; }                     // the subgradient chosen where the power's derivative is infinite
  // dr/dI = -num / den^2, dr/dFP = alpha (I + eps) / den^2, dr/dFN = beta (I + eps) / den^2;  dI = t, dFP = 1 - t, dFN = -t
  const float d2 = den * den;
  a = dv * (cfg.alpha * ie) / d2;
  bc = -dv * fmaf(cfg.alpha + cfg.beta, ie, num) / d2;
}

// One workgroup: the fold of the partials, then thread 0 forms the values [total, Tversky value per term .., focal value, total
// again] and coef [B][C][3].  The class count is a run-time number here: no per-thread arrays, and the same instructions for every C.
__global__ void __launch_bounds__(256) imb_finalize_kernel(float* __restrict__ sums, int nblk, float* __restrict__ values, float* __restrict__ coef,
                                                           const float* __restrict__ base_total, int B, long long S, int C, ImbCfg cfg,
                                                           const float* __restrict__ scale_dev) {
  ls_fold(sums, nblk, B * C * 4, sums);      // B * C * 4 <= 256 partial rows into sums[0 ..)
  if (threadIdx.x != 0) return;
  const float sc = scale_dev ? scale_dev[0] : 1.f;
  const float Bf = (float)B;
  const float wf = sc * cfg.w_focal;
  const float N = (float)B * (float)S;      // divisions below, not products with a rounded reciprocal: one rounding less each
  // the focal term: F weighted by class, in (b, c) order; its coefficient G opens every row of coef
  float F = 0.f;
  for (int b = 0; b < B; ++b) {
#pragma unroll
    for (int c = 0; c < LTU_WIDE_MAXC; ++c) {
      if (c < C) {
        F = fmaf(cfg.a[c], sums[((long long)b * C + c) * 4 + 3], F);
        float* o = coef + ((long long)b * C + c) * 3;
        o[0] = 0.f; o[1] = 0.f; o[2] = -(wf * cfg.a[c]) / N;
      }
    }
  }
  const float fv = F / N;
  float total = base_total ? base_total[0] : 0.f;
#pragma unroll
  for (int k = 0; k < IMB_MAX_K; ++k) {
    if (k < cfg.K) {
      const int c = cfg.cls[k];
      const float wk = sc * cfg.w[k];
      float value = 0.f, v, a, bc;
      if (cfg.batch) {
        float I = 0.f, FP = 0.f, FN = 0.f;
        for (int b = 0; b < B; ++b) {
          const float* sb = sums + ((long long)b * C + c) * 4;
          I += sb[0]; FP += sb[1]; FN += sb[2];
        }
        imb_tversky(I, FP, FN, cfg, v, a, bc);
        value = v;
        for (int b = 0; b < B; ++b) {
          float* o = coef + ((long long)b * C + c) * 3;
          o[0] = fmaf(wk, a, o[0]); o[1] = fmaf(wk, bc, o[1]);
        }
      } else {
        const float wb = wk / Bf;
        for (int b = 0; b < B; ++b) {
          const float* sb = sums + ((long long)b * C + c) * 4;
          imb_tversky(sb[0], sb[1], sb[2], cfg, v, a, bc);
          value += v;
          float* o = coef + ((long long)b * C + c) * 3;
          o[0] = fmaf(wb, a, o[0]); o[1] = fmaf(wb, bc, o[1]);
        }
        value /= Bf;
      }
      values[1 + k] = value;
      total = fmaf(wk, value, total);
    }
  }
  values[1 + cfg.K] = fv;
  total = fmaf(wf, fv, total);
  values[0] = total;
  values[2 + cfg.K] = total;      // a second copy: the differentiable scalar beside the report, no copy kernel
}

// ls_walk_grid (loss_stream.h) for a stage that adds into what an earlier one wrote: the same walk and the same loads, and o arrives
// holding the voxel's dp.  Kept here: the shared walk writes only, and its users are not touched.
template <int C, bool V4, class Grad>
__device__ __forceinline__ void imb_walk_grid_acc(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ dp,
                                                  long long S, Grad grad) {
  const long long base = (long long)blockIdx.y * S;
  if constexpr (V4) {
    for (long long s = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; s < S; s += (long long)gridDim.x * 1024) {
      const long long i = base + s;
      uint32_t labs;
      float f[4 * C], o[4 * C];
      ls_fetch4<C>(p, label, i, labs, f);
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(dp + i * C + 4 * q);
        o[4 * q] = t.x; o[4 * q + 1] = t.y; o[4 * q + 2] = t.z; o[4 * q + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) grad((int)((labs >> (8 * j)) & 255u), f + j * C, o + j * C);
#pragma unroll
      for (int q = 0; q < C; ++q) *reinterpret_cast<float4*>(dp + i * C + 4 * q) = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
  } else {
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < S; s += (long long)gridDim.x * 256) {
      const long long i = base + s;
      float f[C], o[C];
#pragma unroll
      for (int c = 0; c < C; ++c) { f[c] = p[i * C + c]; o[c] = dp[i * C + c]; }
      grad((int)label[i], f, o);
#pragma unroll
      for (int c = 0; c < C; ++c) dp[i * C + c] = o[c];
    }
  }
}

// dp[s, c] (+)= gscale (A + t (Bc + G f'(p))), f' = -gf (1 - p)^(gf - 1) log max(p, 1e-6) + [p > 1e-6] (1 - p)^gf / p, evaluated on
// the label's channel only; Bc + G f' in one fused multiply-add.  V4: four voxels per thread; ACC: added into what dp holds
template <int C, bool V4, bool ACC>
__global__ void __launch_bounds__(256) imb_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, const float* __restrict__ coef,
                                                      float gf, const float* __restrict__ gscale, float* __restrict__ dp, long long S) {
  const float gs = gscale[0];
  const int mode = imb_mode(gf);
  float k0[C], k1[C], k2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* k = coef + ((long long)blockIdx.y * C + c) * 3;
    k0[c] = k[0]; k1[c] = k[1]; k2[c] = k[2];
  }
  auto grad = [&](int lab, const float* f, float* o) {
    float pl = 1.f;
#pragma unroll
    for (int c = 0; c < C; ++c) pl = lab == c ? f[c] : pl;
    const float inv = pl > 1e-6f ? 1.f / pl : 0.f;
    float fp = inv;                                                       // gf == 0: f = log max(p, 1e-6)
    if (mode != 0) {
      const float q = fmaxf(1.f - pl, 0.f);
      const float pw1 = imb_pow1(q, gf, mode);
      fp = pw1 * fmaf(q, inv, ls_rounded(-gf * logf(fmaxf(pl, 1e-6f))));
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float d = gs * (lab == c ? k0[c] + fmaf(k2[c], fp, k1[c]) : k0[c]);
      o[c] = ACC ? o[c] + ls_rounded(d) : d;      // rounded on its own: what the write path would have stored, then one add
    }
  };
  if constexpr (ACC) imb_walk_grid_acc<C, V4>(p, label, dp, S, grad);
  else ls_walk_grid<C, V4>(p, label, dp, S, grad);
}

// ------------------------------------------------------------------------------------------------ host side
static bool imb_shape_ok(int B, long long S, int C) {
  return C >= 2 && C <= LTU_WIDE_MAXC && B >= 1 && S >= 1 && (long long)B * C * 4 <= 256;
}
static bool imb_focal_gamma_ok(float gf) { return gf == 0.f || (gf >= 1.f && gf <= 5.f); }      // NaN fails both

extern "C" long long ltu_loss_imb_ws_floats(int B, long long S, int C) {
  return imb_shape_ok(B, S, C) ? (1 + (long long)cdiv(S, loss_rows(B, S))) * B * C * 4 : 0;
}

extern "C" int ltu_loss_imb_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef,
                                const float* base_total, const int* classes, const float* w, int K, const float* params, float w_focal,
                                float focal_gamma, const float* focal_alpha, const float* scale_dev, int B, long long S, int C,
                                ltu_stream_t s) {
  if (!imb_shape_ok(B, S, C)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || sums == nullptr || values == nullptr || coef == nullptr || params == nullptr) return LTU_E_ARG;
  if (K < 0 || K > IMB_MAX_K || (K > 0 && (classes == nullptr || w == nullptr))) return LTU_E_ARG;
  if (sums_floats < ltu_loss_imb_ws_floats(B, S, C)) return LTU_E_ARG;
  ImbCfg cfg;
  cfg.K = K;
  for (int k = 0; k < IMB_MAX_K; ++k) { cfg.cls[k] = 0; cfg.w[k] = 0.f; }
  for (int k = 0; k < K; ++k) {
    if (classes[k] < 0 || classes[k] >= C || !isfinite(w[k])) return LTU_E_ARG;
    cfg.cls[k] = classes[k];
    cfg.w[k] = w[k];
  }
  const float alpha = params[0], beta = params[1], gamma = params[2], eps = params[3];
  if (!isfinite(alpha) || !isfinite(beta) || !(alpha >= 0.f) || !(beta >= 0.f) || !(alpha + beta > 0.f)) return LTU_E_ARG;
  if (!(gamma >= 1.f && gamma <= 3.f) || !isfinite(eps) || !(eps > 0.f)) return LTU_E_ARG;
  if (params[4] != 0.f && params[4] != 1.f) return LTU_E_ARG;
  if (!isfinite(w_focal) || !imb_focal_gamma_ok(focal_gamma)) return LTU_E_ARG;
  cfg.alpha = alpha; cfg.beta = beta; cfg.inv_gamma = 1.f / gamma; cfg.eps = eps;
  cfg.batch = params[4] != 0.f;
  cfg.w_focal = w_focal;
  for (int c = 0; c < LTU_WIDE_MAXC; ++c) {
    cfg.a[c] = (c < C && focal_alpha) ? focal_alpha[c] : 1.f;
    if (!isfinite(cfg.a[c]) || cfg.a[c] < 0.f) return LTU_E_ARG;
  }
  const long long rows = loss_rows(B, S);
  const int nblk = (int)cdiv(S, rows);
  const bool v4 = loss_v4(S, C);
  const float gf = w_focal != 0.f ? focal_gamma : -1.f;      // without a focal weight the pass skips the log and F stays 0
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(C, {
    if constexpr (CT >= 2) {
      if (v4)
        hipLaunchKernelGGL((imb_sums_kernel<CT, true>), dim3(nblk, B), dim3(256), 0, st, p, label, sums, S, (int)rows, gf);
      else
        hipLaunchKernelGGL((imb_sums_kernel<CT, false>), dim3(nblk, B), dim3(256), 0, st, p, label, sums, S, (int)rows, gf);
    }
  });
  hipLaunchKernelGGL(imb_finalize_kernel, dim3(1), dim3(256), 0, st, sums, nblk, values, coef, base_total, B, S, C, cfg, scale_dev);
  return ltu_check_launch();
}

extern "C" int ltu_loss_imb_bwd(const float* p, const uint8_t* label, const float* coef, long long coef_floats, float focal_gamma,
                                const float* gscale, float* dp, int accumulate, int B, long long S, int C, ltu_stream_t s) {
  if (!imb_shape_ok(B, S, C)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || coef == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  if (coef_floats < (long long)B * C * 3 || !imb_focal_gamma_ok(focal_gamma)) return LTU_E_ARG;
  const bool v4 = loss_v4(S, C);
  const dim3 grid = loss_bwd_grid(B, S, v4);
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(C, {
    if constexpr (CT >= 2) {
      if (v4 && accumulate)
        hipLaunchKernelGGL((imb_bwd_kernel<CT, true, true>), grid, dim3(256), 0, st, p, label, coef, focal_gamma, gscale, dp, S);
      else if (v4)
        hipLaunchKernelGGL((imb_bwd_kernel<CT, true, false>), grid, dim3(256), 0, st, p, label, coef, focal_gamma, gscale, dp, S);
      else if (accumulate)
        hipLaunchKernelGGL((imb_bwd_kernel<CT, false, true>), grid, dim3(256), 0, st, p, label, coef, focal_gamma, gscale, dp, S);
      else
        hipLaunchKernelGGL((imb_bwd_kernel<CT, false, false>), grid, dim3(256), 0, st, p, label, coef, focal_gamma, gscale, dp, S);
    }
  });
  return ltu_check_launch();
}
