// Deep-supervision losses of one decoder level for gfx950, forward + analytic backward.
//
// Reference: loss/criterions.py 696-735 (class-mass-weighted CE on probabilities), 35-70 (per-class
// Dice), 416-442 (balanced Dice); loss/multi_criterions.py 594-615, 58-110 (one-hot variants: identical
// arithmetic once the one-hot target is "label == class"); label pyramid utils/utils_3D_embed_full.py:64,73-76.
//
// Every loss of a level is a function of four per-(sample, class) sums over the S voxels
//     P = sum p_c     T = sum t_c     I = sum p_c t_c     E = sum t_c (1-p_c) log(max(p_c, 1e-6))
// so the forward is one streaming reduction + a tiny finalize, and the backward is one streaming pass
//     dL/dp[s,c] = alpha[b,c] + t_c * (beta[b,c] + gamma[b,c] * f'(p)),   f(p) = (1-p) log(max(p,1e-6))
// with (alpha, beta, gamma) produced by the finalize kernel.
//
// One set of kernels for 1 .. 8 classes behind both entry-point families (ltu_loss_*: C <= 4, nine values; ltu_loss_wide_*:
// 2 <= C <= 8, C + 5 values).  The class count is a template argument everywhere: per-thread arrays are indexed by unrolled
// loops only and stay in registers.
#include "loss_stream.h"

// One voxel into {P, T, I, E} of each class.  The rounding is written out, not left to -ffp-contract=fast (see the finalize kernel):
// t (1 - p) is exact (t is 0 or 1) and meets the E sum in one fused multiply-add with the log.  Left alone, the compiler fuses most
// of these and rounds the product on its own where it has paired it with the product of I into a packed add: which voxels of a
// thread those are changes with the class count and with any edit.  p t is exact, so I is the same number either way; as a fused
// multiply-add it keeps the four-voxel kernel of C = 2 at 62 VGPRs (97, one wave per SIMD less, with p * t and a separate add).
template <int C>
__device__ __forceinline__ void loss_add(int lab, const float* f, float (&acc)[C * 4]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float pc = f[c];
    const float t = lab == c ? 1.f : 0.f;
    acc[c * 4 + 0] += pc;
    acc[c * 4 + 1] += t;
    acc[c * 4 + 2] = fmaf(pc, t, acc[c * 4 + 2]);
    acc[c * 4 + 3] = fmaf(lab == c ? 1.f - pc : 0.f, logf(fmaxf(pc, 1e-6f)), acc[c * 4 + 3]);
  }
}

// p f32 [B][S][C], label u8 [B][S]; sums [1 + block][B][C][4] = {P,T,I,E}.  V4: four voxels per thread and trip, two trips in flight
// up to C = 4 (loss_stream.h)
template <int C, bool V4>
__global__ void __launch_bounds__(256) loss_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ sums,
                                                        long long S, int rows_per_block) {
  float acc[C * 4];
#pragma unroll
  for (int k = 0; k < C * 4; ++k) acc[k] = 0.f;
  ls_walk_block<C, V4, (C <= 4)>(p, label, S, rows_per_block, [&](int lab, const float* f) { loss_add<C>(lab, f, acc); });
  ls_store_partial<C * 4>(acc, sums);
}

// weights: w_ce, w_bal, w_dice[c] (standard per-class Dice on class c), w_fg.  values out: [0] = total, [1] = ce, [2] = bal,
// [3 + c] = dice_c, [fg_slot] = foreground-union dice, [fg_slot + 1] = total again (fg_slot: 7 behind ltu_loss_fwd, 3 + C behind
// ltu_loss_wide_fwd).  coef [B][C][3] = alpha, beta, gamma (already multiplied by the loss weights).
struct LossCfg {
  float w_ce, w_bal, w_dice[LTU_WIDE_MAXC];
  float w_fg;          // Dice of the foreground union, p' = 1 - p_0 against t' = 1 - t_0 (loss/multi_criterions.py:30-56, DiceClassLoss0)
};

// scale_dev (nullable): a device-resident factor applied to all loss weights of this level (the per-epoch deep-supervision weight
// divided by the number of accumulated micro-steps): a captured HIP graph then follows weight changes without being re-captured.
// Where a product meets a sum the rounding is written out, not left to -ffp-contract=fast: fmaf at the sites the compiler fused
// when the class loops were rolled over a run-time C, two rounded products at the one it did not (the first two terms of the
// total).  These are the bits every recorded result carries; left alone, the compiler packs some pairs of products into
// v_pk_mul_f32 and adds them unfused, fuses others, and chooses differently from one class count to the next.
template <int C>
__global__ void __launch_bounds__(256) loss_finalize_kernel(float* __restrict__ sums, int nblk, float* __restrict__ values, float* __restrict__ coef,
                                                            int B, long long S, LossCfg cfg, int fg_slot, const float* __restrict__ scale_dev) {
#pragma clang fp contract(off)
  ls_fold(sums, nblk, B * C * 4, sums);      // B * C * 4 <= 256 partial rows into sums[0 ..)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (scale_dev != nullptr) {
    const float sc = scale_dev[0];
    cfg.w_ce *= sc; cfg.w_bal *= sc; cfg.w_fg *= sc;
#pragma unroll
    for (int c = 0; c < C; ++c) cfg.w_dice[c] *= sc;
  }
  float fg = 0.f;
  float ce = 0.f, bal = 0.f, dice[C];
#pragma unroll
  for (int c = 0; c < C; ++c) dice[c] = 0.f;
  const float Z = (float)B * (float)S * (float)C;
  for (int b = 0; b < B; ++b) {
    const float* sb = sums + (long long)b * C * 4;
    float Ttot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) Ttot += sb[c * 4 + 1];
    // balanced dice pieces
    float num = 0.f, den = 0.f, wc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float t = sb[c * 4 + 1] + 1e-5f;
      wc[c] = 1.f / (t * t);
      num = fmaf(sb[c * 4 + 2], wc[c], num);
      den = fmaf(sb[c * 4 + 0] + sb[c * 4 + 1], wc[c], den);
    }
    const float Nb = 2.f * num + 1e-5f, Db = den + 1e-5f;
    bal += Nb / Db;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float P = sb[c * 4 + 0], T = sb[c * 4 + 1], I = sb[c * 4 + 2], E = sb[c * 4 + 3];
      const float w = (Ttot - (P + 1e-5f)) / Ttot;
      ce = fmaf(-w, E, ce);
      const float N = 2.f * I + 1e-9f, Dd = P + T + 1e-9f;
      dice[c] += N / Dd;
      float alpha = 0.f, beta = 0.f, gamma = 0.f;
      // CE: L = -(1/Z) sum w E  ->  dL/dp = (1/Z) (E/Ttot) - (1/Z) w t f'(p)
      alpha += cfg.w_ce * E / (Z * Ttot);
      gamma += -cfg.w_ce * w / Z;
      // Dice_c: L = 1 - (1/B) N/D -> dL/dp_c = (1/B) N/D^2 - (1/B) 2 t / D
      alpha += cfg.w_dice[c] * N / ((float)B * Dd * Dd);
      beta += -cfg.w_dice[c] * 2.f / ((float)B * Dd);
      // balanced Dice
      alpha += cfg.w_bal * Nb * wc[c] / ((float)B * Db * Db);
      beta += -cfg.w_bal * 2.f * wc[c] / ((float)B * Db);
      if (c == 0) {
        // foreground union: P' = S - P, T' = S - T, I' = S - P - T + I;  L = 1 - (1/B) N'/D', N' = 2 I' + eps, D' = P' + T' + eps
        //   dL/dp_0 = (1/B) (2 (1 - t_0) / D' - N' / D'^2)
        const float Sf = (float)S;
        const float Nf = 2.f * (Sf - P - T + I) + 1e-9f, Df = (Sf - P) + (Sf - T) + 1e-9f;
        fg += Nf / Df;
        alpha += cfg.w_fg * (2.f / Df - Nf / (Df * Df)) / (float)B;
        beta += -cfg.w_fg * 2.f / ((float)B * Df);
      }
      float* o = coef + ((long long)b * C + c) * 3;
      o[0] = alpha; o[1] = beta; o[2] = gamma;
    }
  }
  ce /= Z;
  bal = 1.f - bal / (float)B;
  // two products and a sum: the pragma does not reach the backend, which fuses one product into the sum unless both are hidden from it
  float t_ce = cfg.w_ce * ce, t_bal = cfg.w_bal * bal;
  asm volatile("" : "+v"(t_ce), "+v"(t_bal));
  float total = t_ce + t_bal;
  values[1] = ce;
  values[2] = bal;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float dv = 1.f - dice[c] / (float)B;
    values[3 + c] = dv;
    total = fmaf(cfg.w_dice[c], dv, total);
  }
  const float fgv = 1.f - fg / (float)B;
  values[fg_slot] = fgv;
  total = fmaf(cfg.w_fg, fgv, total);
  values[0] = total;
  values[fg_slot + 1] = total;      // a second copy: the autograd wrapper exposes it as the differentiable scalar and the rest as the report
}

// dp[s,c] = gscale * (alpha + t (beta + gamma f'(p))), beta + gamma f' in one fused multiply-add.  V4: four voxels per thread
template <int C, bool V4>
__global__ void __launch_bounds__(256) loss_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, const float* __restrict__ coef,
                                                       const float* __restrict__ gscale, float* __restrict__ dp, long long S) {
  const float gs = gscale[0];
  float k0[C], k1[C], k2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* k = coef + ((long long)blockIdx.y * C + c) * 3;
    k0[c] = k[0]; k1[c] = k[1]; k2[c] = k[2];
  }
  ls_walk_grid<C, V4>(p, label, dp, S, [&](int lab, const float* f, float* o) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float pc = f[c];
      const float fp = -logf(fmaxf(pc, 1e-6f)) + (pc > 1e-6f ? (1.f - pc) / pc : 0.f);
      o[c] = gs * (lab == c ? k0[c] + fmaf(k2[c], fp, k1[c]) : k0[c]);
    }
  });
}

// ------------------------------------------------------------------------------------------------ host side
// Both entry-point families end here.  w_dice: C Dice weights (NULL: all zero); fg_slot: where the values hold the union Dice (the
// second total follows it).
static int loss_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B, long long S, int C,
                    float w_ce, float w_bal, const float* w_dice, float w_fg, int fg_slot, const float* scale_dev, ltu_stream_t s) {
  const long long rows = loss_rows(B, S);
  const int nblk = (int)cdiv(S, rows);
  if ((1 + (long long)nblk) * B * C * 4 > sums_floats) return LTU_E_ARG;          // the scratch is shorter than this geometry needs
  LossCfg cfg;
  cfg.w_ce = w_ce; cfg.w_bal = w_bal; cfg.w_fg = w_fg;
  for (int c = 0; c < LTU_WIDE_MAXC; ++c) cfg.w_dice[c] = (c < C && w_dice) ? w_dice[c] : 0.f;
  const bool v4 = loss_v4(S, C);
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(C, {
    if (v4) {          // implies C >= 2: no four-voxel kernel is instantiated for one class
      if constexpr (CT >= 2) hipLaunchKernelGGL((loss_sums_kernel<CT, true>), dim3(nblk, B), dim3(256), 0, st, p, label, sums, S, (int)rows);
    } else {
      hipLaunchKernelGGL((loss_sums_kernel<CT, false>), dim3(nblk, B), dim3(256), 0, st, p, label, sums, S, (int)rows);
    }
    hipLaunchKernelGGL(loss_finalize_kernel<CT>, dim3(1), dim3(256), 0, st, sums, nblk, values, coef, B, S, cfg, fg_slot, scale_dev);
  });
  return ltu_check_launch();
}
static int loss_bwd(const float* p, const uint8_t* label, const float* coef, const float* gscale, float* dp, int B, long long S, int C,
                    ltu_stream_t s) {
  const bool v4 = loss_v4(S, C);
  const dim3 grid = loss_bwd_grid(B, S, v4);
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(C, {
    if (v4) {
      if constexpr (CT >= 2) hipLaunchKernelGGL((loss_bwd_kernel<CT, true>), grid, dim3(256), 0, st, p, label, coef, gscale, dp, S);
    } else {
      hipLaunchKernelGGL((loss_bwd_kernel<CT, false>), grid, dim3(256), 0, st, p, label, coef, gscale, dp, S);
    }
  });
  return ltu_check_launch();
}


// 1 <= C <= 4: five Dice weights (classes 0 .. 3, union; NULL: all zero), nine values (union Dice at [7], second total at [8])
extern "C" long long ltu_loss_ws_floats(int B, long long S, int C) { return (1 + cdiv(S, loss_rows(B, S))) * (long long)B * C * 4; }

extern "C" int ltu_loss_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B, long long S,
                            int C,
                            float w_ce, float w_bal, const float* w_dice, const float* scale_dev, ltu_stream_t s) {
  if (C < 1 || C > 4 || B * C * 4 > 256) return LTU_E_SHAPE;
  return loss_fwd(p, label, sums, sums_floats, values, coef, B, S, C, w_ce, w_bal, w_dice, w_dice ? w_dice[4] : 0.f, 7, scale_dev, s);
}

extern "C" int ltu_loss_bwd(const float* p, const uint8_t* label, const float* coef, const float* gscale, float* dp, int B,
                            long long S, int C, ltu_stream_t s) {
  if (C > 4) return ltu_loss_wide_bwd(p, label, coef, gscale, dp, B, S, C, s);      // coefficients of ltu_loss_wide_fwd
  return loss_bwd(p, label, coef, gscale, dp, B, S, C, s);
}

// 2 <= C <= 8: C + 1 Dice weights (every class, then the union), C + 5 values (union Dice at [3 + C], second total at [4 + C])
static bool loss_wide_shape_ok(int B, long long S, int C) {
  return C >= 2 && C <= LTU_WIDE_MAXC && B >= 1 && S >= 1 && (long long)B * C * 4 <= 256;
}
extern "C" long long ltu_loss_wide_ws_floats(int B, long long S, int C) { return loss_wide_shape_ok(B, S, C) ? ltu_loss_ws_floats(B, S, C) : 0; }

extern "C" int ltu_loss_wide_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B,
                                 long long S, int C, float w_ce, float w_bal, const float* w_dice, const float* scale_dev, ltu_stream_t s) {
  if (!loss_wide_shape_ok(B, S, C)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || sums == nullptr || values == nullptr || coef == nullptr || w_dice == nullptr) return LTU_E_ARG;
  return loss_fwd(p, label, sums, sums_floats, values, coef, B, S, C, w_ce, w_bal, w_dice, w_dice[C], 3 + C, scale_dev, s);
}

extern "C" int ltu_loss_wide_bwd(const float* p, const uint8_t* label, const float* coef, const float* gscale, float* dp, int B, long long S,
                                 int C, ltu_stream_t s) {
  if (!loss_wide_shape_ok(B, S, C)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || coef == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  return loss_bwd(p, label, coef, gscale, dp, B, S, C, s);
}

// label pyramid: u8 [B][H][W][D] -> max over (2,2,kd) windows, kd in {1,2}
__global__ void label_maxpool_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, int B, int H, int W, int D, int kd) {
  const int Ho = H / 2, Wo = W / 2, Do = D / kd;
  const long long n = (long long)B * Ho * Wo * Do;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % Do);
    long long t = i / Do;
    const int w = (int)(t % Wo); t /= Wo;
    const int h = (int)(t % Ho);
    const int b = (int)(t / Ho);
    uint8_t m = 0;
    for (int a = 0; a < 2; ++a)
      for (int e = 0; e < 2; ++e)
        for (int f = 0; f < kd; ++f) {
          const uint8_t v = x[(((long long)b * H + 2 * h + a) * W + 2 * w + e) * D + d * kd + f];
          m = v > m ? v : m;
        }
    y[i] = m;
  }
}
extern "C" int ltu_label_maxpool(const uint8_t* x, uint8_t* y, int B, int H, int W, int D, int kd, ltu_stream_t s) {
  if ((kd != 1 && kd != 2) || H % 2 || W % 2 || D % kd) return LTU_E_SHAPE;
  const long long n = (long long)B * (H / 2) * (W / 2) * (D / kd);
  long long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(label_maxpool_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, x, y, B, H, W, D, kd);
  return ltu_check_launch();
}
