// Region-based training (nnU-Net's region_class_order): R <= 8 overlapping label regions, one sigmoid channel each.  Region r is the
// set of u8 label values members[r]; a voxel's membership of all regions is one byte, bits = lut[label] with lut[v] = sum_r [v in
// members[r]] << r (a label in no region is background for every channel).  This file holds
//   - the bit-mask of a label volume and its pyramid: a bitwise OR over the (2, 2, kd) windows of ltu_label_maxpool, which max-pools
//     every region's indicator on its own (a max of the raw label would be wrong for regions that are not nested in label order);
//   - the sixth stage of a level's loss chain: binary cross-entropy and Dice per region on the sigmoid probabilities;
//   - the way back: a label map painted from the probabilities in region order, and TP / FP / FN counts per (sample, region).
// The loss stage.  With t_r = (bits >> r) & 1 the sums pass accumulates, per (sample, region) and each directly,
//     I = sum p t     FP = sum p (1 - t)     FN = sum t (1 - p)     E = sum -[t log max(p, 1e-6) + (1 - t) log max(1 - p, 1e-6)]
// FP and FN are never formed as P - I and T - I (loss_imbalance.hip says why: late in training the subtraction cancels and can come
// out negative).  p t and p (1 - t) are exact, t (1 - p) is one rounded difference, and E takes one log per (voxel, region).
//     BCE  = sum_{b, r} E / (B S R)
//     D_r  = (FP + FN) / (2 I + FP + FN + 2 eps)      batch: I, FP, FN summed over b first;  else the mean over b of the sample's ratio
//     Dice = (1 / R) sum_r D_r          (D_r is the Tversky term of loss_imbalance.hip at alpha = beta = 0.5 with the same eps)
//     total = before + scale (w_bce BCE + w_dice Dice)
// and every gradient has the form  dp[b, s, r] = gscale (A[b, r] + t Bc[b, r] + G[b, r] e'(p, t)),  coef [B][R][3] = (A, Bc, G)
// written by the finalize kernel, already weighted and scaled.  e' is the derivative of the clamped expression: -1 / p where t = 1
// and p > 1e-6, 1 / (1 - p) where t = 0 and 1 - p > 1e-6, 0 otherwise.
// nnU-Net applies its BCE to the logits (BCEWithLogitsLoss); on probabilities clamped at 1e-6 the two differ only where |z| >
// 13.8 (sigmoid(-13.8) = 1e-6), where this term and its gradient stay bounded.
// Built on loss_stream.h, the bit-mask byte in the label's place: per-workgroup partials folded in a fixed order, no floating-point
// atomics, no host read, no allocation.  Two calls agree bit for bit and the stage can be captured.
#include "loss_stream.h"

#include <math.h>

#define REG_MAXR 8

struct RegionLut { uint8_t v[256]; };
struct RegionOrder { uint8_t v[REG_MAXR]; };

// ------------------------------------------------------------------------------------------------ bit-mask and pyramid
__global__ void __launch_bounds__(256) region_bits_kernel(const uint8_t* __restrict__ label, const RegionLut lut, uint8_t* __restrict__ out,
                                                          long long n) {
  __shared__ uint8_t tab[256];
  tab[threadIdx.x] = lut.v[threadIdx.x];
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = tab[label[i]];
}

// u8 [B][H][W][D] -> bitwise OR over (2, 2, kd) windows, kd in {1, 2}: the walk of label_maxpool_kernel (loss.hip)
__global__ void __launch_bounds__(256) bits_orpool_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, int B, int H, int W, int D,
                                                          int kd) {
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
        for (int f = 0; f < kd; ++f) m |= x[(((long long)b * H + 2 * h + a) * W + 2 * w + e) * D + d * kd + f];
    y[i] = m;
  }
}

static unsigned region_grid(long long n) {
  long long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

extern "C" int ltu_region_bits(const uint8_t* label, const uint8_t* lut, uint8_t* out, long long n, ltu_stream_t s) {
  if (n < 1) return LTU_E_SHAPE;
  if (label == nullptr || lut == nullptr || out == nullptr) return LTU_E_ARG;
  RegionLut t;
  memcpy(t.v, lut, 256);      // lut is host memory: the table travels by value with the launch
  hipLaunchKernelGGL(region_bits_kernel, dim3(region_grid(n)), dim3(256), 0, (hipStream_t)s, label, t, out, n);
  return ltu_check_launch();
}

extern "C" int ltu_bits_orpool(const uint8_t* x, uint8_t* y, int B, int H, int W, int D, int kd, ltu_stream_t s) {
  if ((kd != 1 && kd != 2) || B < 1 || H < 2 || W < 2 || D < kd || H % 2 || W % 2 || D % kd) return LTU_E_SHAPE;
  if (x == nullptr || y == nullptr) return LTU_E_ARG;
  const long long n = (long long)B * (H / 2) * (W / 2) * (D / kd);
  hipLaunchKernelGGL(bits_orpool_kernel, dim3(region_grid(n)), dim3(256), 0, (hipStream_t)s, x, y, B, H, W, D, kd);
  return ltu_check_launch();
}

// ------------------------------------------------------------------------------------------------ the loss stage
// One voxel into {I, FP, FN, E} of each region
template <int R>
__device__ __forceinline__ void reg_add(int bits, const float* f, float (&acc)[R * 4]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float pr = f[r];
    const bool t = (bits >> r) & 1;
    const float q = 1.f - pr;
    acc[r * 4 + 0] += t ? pr : 0.f;
    acc[r * 4 + 1] += t ? 0.f : pr;
    acc[r * 4 + 2] += t ? q : 0.f;
    acc[r * 4 + 3] -= logf(fmaxf(t ? pr : q, 1e-6f));
  }
}

// p f32 [B][S][R], bits u8 [B][S]; sums [1 + block][B][R][4] = {I, FP, FN, E}.  V4: four voxels per thread and trip, two trips in
// flight up to R = 4 (loss_stream.h)
template <int R, bool V4>
__global__ void __launch_bounds__(256) region_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ bits, float* __restrict__ sums,
                                                          long long S, int rows_per_block) {
  float acc[R * 4];
#pragma unroll
  for (int k = 0; k < R * 4; ++k) acc[k] = 0.f;
  ls_walk_block<R, V4, (R <= 4)>(p, bits, S, rows_per_block, [&](int b, const float* f) { reg_add<R>(b, f, acc); });
  ls_store_partial<R * 4>(acc, sums);
}

// D = (FP + FN) / (2 I + FP + FN + 2 eps) and its derivative as the two coefficients of a voxel, dD/dp = a + t bc:
// dD/dFP = dD/dFN = (2 I + 2 eps) / den^2, dD/dI = -2 (FP + FN) / den^2;  dI = t, dFP = 1 - t, dFN = -t
__device__ __forceinline__ void reg_dice(float I, float FP, float FN, float eps, float& v, float& a, float& bc) {
  const float num = FP + FN;
  const float ie = fmaf(2.f, I, 2.f * eps);
  const float den = ie + num;
  v = num / den;
  a = ie / (den * den);
  bc = -2.f / den;
}

// One workgroup: the fold of the partials, then thread 0 forms values [R + 4] = {total, BCE, Dice, D_0 .. D_{R-1}, total again} and
// coef [B][R][3].  The region count is a run-time number here, as the class count is in imb_finalize_kernel.
__global__ void __launch_bounds__(256) region_finalize_kernel(float* __restrict__ sums, int nblk, float* __restrict__ values, float* __restrict__ coef,
                                                              const float* __restrict__ base_total, int B, long long S, int R, float w_bce,
                                                              float w_dice, int batch, float eps, const float* __restrict__ scale_dev) {
  ls_fold(sums, nblk, B * R * 4, sums);      // B * R * 4 <= 256 partial rows into sums[0 ..)
  if (threadIdx.x != 0) return;
  const float sc = scale_dev ? scale_dev[0] : 1.f;
  const float wb = sc * w_bce, wd = sc * w_dice;
  const float Bf = (float)B, Rf = (float)R;
  const float N = (float)B * (float)S * Rf;
  const float G = wb / N;
  float E = 0.f;
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < R; ++r) E += sums[((long long)b * R + r) * 4 + 3];
  const float bce = E / N;
  float dice = 0.f;
  for (int r = 0; r < R; ++r) {
    float value = 0.f, v, a, bc;
    if (batch) {
      float I = 0.f, FP = 0.f, FN = 0.f;
      for (int b = 0; b < B; ++b) {
        const float* sb = sums + ((long long)b * R + r) * 4;
        I += sb[0]; FP += sb[1]; FN += sb[2];
      }
      reg_dice(I, FP, FN, eps, v, a, bc);
      value = v;
      const float wr = wd / Rf;
      for (int b = 0; b < B; ++b) {
        float* o = coef + ((long long)b * R + r) * 3;
        o[0] = ls_rounded(wr * a); o[1] = ls_rounded(wr * bc); o[2] = G;
      }
    } else {
      const float wr = wd / (Rf * Bf);
      for (int b = 0; b < B; ++b) {
        const float* sb = sums + ((long long)b * R + r) * 4;
        reg_dice(sb[0], sb[1], sb[2], eps, v, a, bc);
        value += v;
        float* o = coef + ((long long)b * R + r) * 3;
        o[0] = ls_rounded(wr * a); o[1] = ls_rounded(wr * bc); o[2] = G;
      }
      value /= Bf;
    }
    values[3 + r] = value;
    dice += value;
  }
  dice /= Rf;
  float total = base_total ? base_total[0] : 0.f;
  total = fmaf(wb, bce, total);
  total = fmaf(wd, dice, total);
  values[0] = total;
  values[1] = bce;
  values[2] = dice;
  values[3 + R] = total;      // a second copy: the differentiable scalar beside the report, no copy kernel
}

// ls_walk_grid (loss_stream.h) for a call that adds into what dp holds: the same walk and the same loads, and o arrives holding the
// voxel's dp (as loss_imbalance.hip and loss_boundary.hip keep theirs)
template <int R, bool V4, class Grad>
__device__ __forceinline__ void reg_walk_grid_acc(const float* __restrict__ p, const uint8_t* __restrict__ bits, float* __restrict__ dp, long long S,
                                                  Grad grad) {
  const long long base = (long long)blockIdx.y * S;
  if constexpr (V4) {
    for (long long s = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; s < S; s += (long long)gridDim.x * 1024) {
      const long long i = base + s;
      uint32_t labs;
      float f[4 * R], o[4 * R];
      ls_fetch4<R>(p, bits, i, labs, f);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(dp + i * R + 4 * q);
        o[4 * q] = t.x; o[4 * q + 1] = t.y; o[4 * q + 2] = t.z; o[4 * q + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) grad((int)((labs >> (8 * j)) & 255u), f + j * R, o + j * R);
#pragma unroll
      for (int q = 0; q < R; ++q) *reinterpret_cast<float4*>(dp + i * R + 4 * q) = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
  } else {
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < S; s += (long long)gridDim.x * 256) {
      const long long i = base + s;
      float f[R], o[R];
#pragma unroll
      for (int r = 0; r < R; ++r) { f[r] = p[i * R + r]; o[r] = dp[i * R + r]; }
      grad((int)bits[i], f, o);
#pragma unroll
      for (int r = 0; r < R; ++r) dp[i * R + r] = o[r];
    }
  }
}

// dp[s, r] (+)= gscale (A + t Bc + G e'(p, t)): the two Dice coefficients meet in one sum, then one fused multiply-add with e'.
// V4: four voxels per thread; ACC: added into what dp holds
template <int R, bool V4, bool ACC>
__global__ void __launch_bounds__(256) region_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ bits, const float* __restrict__ coef,
                                                         const float* __restrict__ gscale, float* __restrict__ dp, long long S) {
  const float gs = gscale[0];
  float k0[R], k1[R], k2[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float* k = coef + ((long long)blockIdx.y * R + r) * 3;
    k0[r] = k[0]; k1[r] = k[0] + k[1]; k2[r] = k[2];
  }
  auto grad = [&](int b, const float* f, float* o) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float pr = f[r], q = 1.f - pr;
      const bool t = (b >> r) & 1;
      const float e = t ? (pr > 1e-6f ? -1.f / pr : 0.f) : (q > 1e-6f ? 1.f / q : 0.f);
      const float d = gs * fmaf(k2[r], e, t ? k1[r] : k0[r]);
      o[r] = ACC ? o[r] + ls_rounded(d) : d;      // rounded on its own: what the write path would have stored, then one add
    }
  };
  if constexpr (ACC) reg_walk_grid_acc<R, V4>(p, bits, dp, S, grad);
  else ls_walk_grid<R, V4>(p, bits, dp, S, grad);
}

// ------------------------------------------------------------------------------------------------ host side of the stage
static bool region_shape_ok(int B, long long S, int R) {
  return R >= 1 && R <= REG_MAXR && B >= 1 && S >= 1 && (long long)B * R * 4 <= 256;
}
// the four-voxel kernels also need their 16-byte and 4-byte loads aligned: a view at an odd offset takes the scalar kernels
static bool region_v4(long long S, int R, const void* p, const void* bits, const void* dp) {
  return loss_v4(S, R) && (uintptr_t)p % 16 == 0 && (uintptr_t)bits % 4 == 0 && (uintptr_t)dp % 16 == 0;
}

extern "C" long long ltu_loss_region_ws_floats(int B, long long S, int R) {
  return region_shape_ok(B, S, R) ? (1 + (long long)cdiv(S, loss_rows(B, S))) * B * R * 4 : 0;
}

extern "C" int ltu_loss_region_fwd(const float* p, const uint8_t* bits, float* sums, long long sums_floats, float* values, float* coef,
                                   const float* base_total, float w_bce, float w_dice, int batch, float eps, const float* scale_dev, int B,
                                   long long S, int R, ltu_stream_t s) {
  if (!region_shape_ok(B, S, R)) return LTU_E_SHAPE;
  if (p == nullptr || bits == nullptr || sums == nullptr || values == nullptr || coef == nullptr) return LTU_E_ARG;
  if (sums_floats < ltu_loss_region_ws_floats(B, S, R)) return LTU_E_ARG;
  if (!isfinite(w_bce) || !isfinite(w_dice) || !isfinite(eps) || !(eps > 0.f) || (batch != 0 && batch != 1)) return LTU_E_ARG;
  const long long rows = loss_rows(B, S);
  const int nblk = (int)cdiv(S, rows);
  const bool v4 = region_v4(S, R, p, bits, nullptr);
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(R, {
    if (v4) hipLaunchKernelGGL((region_sums_kernel<CT, true>), dim3(nblk, B), dim3(256), 0, st, p, bits, sums, S, (int)rows);
    else hipLaunchKernelGGL((region_sums_kernel<CT, false>), dim3(nblk, B), dim3(256), 0, st, p, bits, sums, S, (int)rows);
  });
  hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(256), 0, st, sums, nblk, values, coef, base_total, B, S, R, w_bce, w_dice, batch,
                     eps, scale_dev);
  return ltu_check_launch();
}

extern "C" int ltu_loss_region_bwd(const float* p, const uint8_t* bits, const float* coef, long long coef_floats, const float* gscale, float* dp,
                                   int accumulate, int B, long long S, int R, ltu_stream_t s) {
  if (!region_shape_ok(B, S, R)) return LTU_E_SHAPE;
  if (p == nullptr || bits == nullptr || coef == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  if (coef_floats < (long long)B * R * 3) return LTU_E_ARG;
  const bool v4 = region_v4(S, R, p, bits, dp);
  const dim3 grid = loss_bwd_grid(B, S, v4);
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(R, {
    if (v4 && accumulate) hipLaunchKernelGGL((region_bwd_kernel<CT, true, true>), grid, dim3(256), 0, st, p, bits, coef, gscale, dp, S);
    else if (v4) hipLaunchKernelGGL((region_bwd_kernel<CT, true, false>), grid, dim3(256), 0, st, p, bits, coef, gscale, dp, S);
    else if (accumulate) hipLaunchKernelGGL((region_bwd_kernel<CT, false, true>), grid, dim3(256), 0, st, p, bits, coef, gscale, dp, S);
    else hipLaunchKernelGGL((region_bwd_kernel<CT, false, false>), grid, dim3(256), 0, st, p, bits, coef, gscale, dp, S);
  });
  return ltu_check_launch();
}

// ------------------------------------------------------------------------------------------------ back to labels, and scoring
// p f32, channels-last [B][N][R] (planes == 0) or planes [B][R][N]: sample b, region r, voxel i at ...
__device__ __forceinline__ float reg_prob(const float* __restrict__ p, int planes, long long b, long long i, int r, long long N, int R) {
  return planes ? p[(b * R + r) * N + i] : p[(b * N + i) * R + r];
}

// nnU-Net's rule: the label starts at 0; for r = 0 .. R-1 in order, order[r] is written where p_r > thr (a later region wins)
__global__ void __launch_bounds__(256) region_labels_kernel(const float* __restrict__ p, int planes, const RegionOrder order, float thr,
                                                            uint8_t* __restrict__ out, long long BN, long long N, int R) {
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < BN; j += (long long)gridDim.x * 256) {
    const long long b = j / N, i = j - b * N;
    uint8_t lab = 0;
#pragma unroll
    for (int r = 0; r < REG_MAXR; ++r)
      if (r < R && reg_prob(p, planes, b, i, r, N, R) > thr) lab = order.v[r];
    out[j] = lab;
  }
}

// the bit-mask of thresholded probabilities: bit r = [p_r > thr]
__global__ void __launch_bounds__(256) region_prob_bits_kernel(const float* __restrict__ p, int planes, float thr, uint8_t* __restrict__ out,
                                                               long long BN, long long N, int R) {
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < BN; j += (long long)gridDim.x * 256) {
    const long long b = j / N, i = j - b * N;
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < REG_MAXR; ++r)
      if (r < R && reg_prob(p, planes, b, i, r, N, R) > thr) m |= 1u << r;
    out[j] = (uint8_t)m;
  }
}

// counts i64 [B][R][3] = {TP, FP, FN}, zero on entry: per-thread counters, the block's meet in LDS, one integer atomic per counter
// and block.  Grid (blocks, B)
__global__ void __launch_bounds__(256) region_counts_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                            unsigned long long* __restrict__ counts, long long N, int R) {
  __shared__ unsigned int blk[REG_MAXR * 3];
  if (threadIdx.x < REG_MAXR * 3) blk[threadIdx.x] = 0u;
  __syncthreads();
  unsigned int c[REG_MAXR * 3];
#pragma unroll
  for (int k = 0; k < REG_MAXR * 3; ++k) c[k] = 0u;
  const long long base = (long long)blockIdx.y * N;
  const long long per = (N + gridDim.x - 1) / gridDim.x;      // at most 2^31 voxels a block: 32-bit counters cannot wrap
  const long long i0 = (long long)blockIdx.x * per;
  const long long i1 = i0 + per < N ? i0 + per : N;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const unsigned a = pred[base + i], t = truth[base + i];
    const unsigned tp = a & t, fp = a & ~t, fn = ~a & t;
#pragma unroll
    for (int r = 0; r < REG_MAXR; ++r) {
      c[r * 3 + 0] += (tp >> r) & 1u;
      c[r * 3 + 1] += (fp >> r) & 1u;
      c[r * 3 + 2] += (fn >> r) & 1u;
    }
  }
#pragma unroll
  for (int k = 0; k < REG_MAXR * 3; ++k)
    if (c[k]) atomicAdd(&blk[k], c[k]);
  __syncthreads();
  if ((int)threadIdx.x < R * 3 && blk[threadIdx.x]) atomicAdd(counts + (long long)blockIdx.y * R * 3 + threadIdx.x, (unsigned long long)blk[threadIdx.x]);
}

// Dice = 2 TP / (2 TP + FP + FN), 1 where both sides are empty (BraTS's convention); formed in double, stored as f32
__global__ void __launch_bounds__(256) region_dice_kernel(const unsigned long long* __restrict__ counts, float* __restrict__ dice, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const unsigned long long tp = counts[k * 3], fp = counts[k * 3 + 1], fn = counts[k * 3 + 2];
  const unsigned long long den = 2 * tp + fp + fn;
  dice[k] = den ? (float)((double)(2 * tp) / (double)den) : 1.f;
}

static bool region_vol_ok(int B, long long N, int R) {
  return R >= 1 && R <= REG_MAXR && B >= 1 && N >= 1 && B <= 65535;
}

extern "C" int ltu_region_labels(const float* p, int planes, const int* class_order, float thr, uint8_t* out, int B, long long N, int R,
                                 ltu_stream_t s) {
  if (!region_vol_ok(B, N, R)) return LTU_E_SHAPE;
  if (p == nullptr || class_order == nullptr || out == nullptr || (planes != 0 && planes != 1) || thr != thr) return LTU_E_ARG;
  RegionOrder o;
  for (int r = 0; r < REG_MAXR; ++r) {
    if (r < R && (class_order[r] < 0 || class_order[r] > 255)) return LTU_E_ARG;
    o.v[r] = r < R ? (uint8_t)class_order[r] : 0;
  }
  hipLaunchKernelGGL(region_labels_kernel, dim3(region_grid(B * N)), dim3(256), 0, (hipStream_t)s, p, planes, o, thr, out, B * N, N, R);
  return ltu_check_launch();
}

extern "C" int ltu_region_prob_bits(const float* p, int planes, float thr, uint8_t* out, int B, long long N, int R, ltu_stream_t s) {
  if (!region_vol_ok(B, N, R)) return LTU_E_SHAPE;
  if (p == nullptr || out == nullptr || (planes != 0 && planes != 1) || thr != thr) return LTU_E_ARG;
  hipLaunchKernelGGL(region_prob_bits_kernel, dim3(region_grid(B * N)), dim3(256), 0, (hipStream_t)s, p, planes, thr, out, B * N, N, R);
  return ltu_check_launch();
}

extern "C" int ltu_region_counts(const uint8_t* pred_bits, const uint8_t* true_bits, long long* counts, float* dice, int B, long long N, int R,
                                 ltu_stream_t s) {
  if (!region_vol_ok(B, N, R)) return LTU_E_SHAPE;
  if (pred_bits == nullptr || true_bits == nullptr || counts == nullptr || dice == nullptr) return LTU_E_ARG;
  long long blocks = (N + 4095) / 4096;      // 16 voxels a thread; at N > 2^31 * 1024 a block's 32-bit counters could wrap: far past any scan
  if (blocks > 1024) blocks = 1024;
  if ((N + blocks - 1) / blocks > 0x7fffffffLL) return LTU_E_SHAPE;
  hipLaunchKernelGGL(region_counts_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)s, pred_bits, true_bits,
                     (unsigned long long*)counts, N, R);
  hipLaunchKernelGGL(region_dice_kernel, dim3(cdiv(B * R, 256)), dim3(256), 0, (hipStream_t)s, (const unsigned long long*)counts, dice, B * R);
  return ltu_check_launch();
}
