// Multi-class evaluation metrics of inference_multi_classes.py:153 and utils_3D_multi_class.py:146-208 (loss/multi_criterions.py:
// DiceClassLoss0 30-56, DiceClassLoss / DiceClassLoss2 58-110, LocalizationLoss 219-281, Recall / Recall2 320-375, Precision /
// Precision2 406-462) and the driver's label map (argmax(predict2, 1), line 158), from one read of the votes.
//
// 1. ltu_class_metrics_pass streams pred f32 [B][C][H][W][D] and target u8 [B][H][W][D] once.  Per (sample b, row h) it sums over
//    (W, D), for every class c: p_c, [t == c], p_c [t == c], and for the foreground union: 1 - p_0, [t != 0], (1 - p_0) [t != 0]
//    (p = the value as given, or [p >= thr] when thr >= 0, the convention of seg_row_sums_kernel).  A row is split into chunks so
//    that even B = 1 launches enough workgroups for the whole chip; each lane accumulates fp32 over at most 2^16 elements and a
//    wave over at most 2^22 (integer-valued sums stay exact), the four waves of a workgroup are folded in fp64 and stored as the
//    chunk's partial: no atomics.  Optionally the same pass writes the arg-max over C as a u8 label map (first maximal index
//    on ties, as torch.argmax).
// 2. ltu_class_metrics_finalize folds the partials in a fixed order in fp64 (one workgroup) and writes the metrics per sample and
//    their batch means; two calls give bit-identical results.
#include "common.h"

#include <math.h>

#define CM_MAX_C 8
#define CM_TARGET_WGS 2048                 // 8 workgroups of 256 lanes per CU on 256 CUs
#define CM_MIN_CHUNK 4096                  // a chunk gives every lane at least 4 float4 steps
#define CM_MAX_CHUNK (256LL << 16)         // 2^16 elements per lane: exact integer-valued fp32 lane partials

// chunks per row of WD elements and their length (a multiple of 4 when the row is)
static void cm_geometry(int B, int H, long long WD, long long* nch, long long* chunk) {
  const long long rows = (long long)B * H;
  long long n = (CM_TARGET_WGS + rows - 1) / rows;
  const long long most = (WD + CM_MIN_CHUNK - 1) / CM_MIN_CHUNK, least = (WD + CM_MAX_CHUNK - 1) / CM_MAX_CHUNK;
  if (n > most) n = most;
  if (n < least) n = least;
  if (n < 1) n = 1;
  long long len = (WD + n - 1) / n;
  len = (len + 3) / 4 * 4;
  *chunk = len;
  *nch = (WD + len - 1) / len;
}

static bool cm_shape_ok(int B, int C, int H, int W, int D) {
  return B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && D > 0 && C >= 2 && C <= CM_MAX_C;
}

// part [B][NS][H][nch] doubles, NS = 3C + 3: s = c (sum p_c), C + c (sum [t == c]), 2C + c (sum p_c [t == c]), 3C (sum 1 - p_0),
// 3C + 1 (sum [t != 0]), 3C + 2 (sum (1 - p_0) [t != 0]).  grid = (nch, H, B); V = elements per lane per step (4: float4 loads of
// pred, one 32-bit load of 4 labels, rows a multiple of 4 and 16-byte aligned planes; 1: any row length).
template <int C, int V>
__global__ void __launch_bounds__(256) cm_stats_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ target,
                                                       uint8_t* __restrict__ lmap, double* __restrict__ part, int H, long long WD,
                                                       long long chunk, float thr) {
  constexpr int NS = 3 * C + 3;
  const int k = blockIdx.x, h = blockIdx.y, b = blockIdx.z, nch = gridDim.x;
  const long long plane = (long long)H * WD;
  const long long row = (long long)b * H + h;
  const float* p = pred + ((long long)b * C * H + h) * WD;
  const uint8_t* t = target + row * WD;
  uint8_t* lm = lmap == nullptr ? nullptr : lmap + row * WD;
  const long long lo = (long long)k * chunk, hi = lo + chunk < WD ? lo + chunk : WD;
  const bool th = thr >= 0.f;
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.f;
  for (long long i = lo + (long long)V * threadIdx.x; i < hi; i += V * 256) {
    float v[C][V];
    uint8_t lab[V];
    if constexpr (V == 4) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float4 x = *reinterpret_cast<const float4*>(p + c * plane + i);
        v[c][0] = x.x; v[c][1] = x.y; v[c][2] = x.z; v[c][3] = x.w;
      }
      const uint32_t w = *reinterpret_cast<const uint32_t*>(t + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) lab[j] = (uint8_t)(w >> (8 * j));
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][0] = p[c * plane + i];
      lab[0] = t[i];
    }
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float best = v[0][j];
      int arg = 0;
      float q0 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float x = v[c][j];
        if (c > 0 && x > best) { best = x; arg = c; }          // strict: the first maximal index wins a tie
        const float q = th ? (x >= thr ? 1.f : 0.f) : x;
        const bool m = lab[j] == c;
        acc[c] += q;
        acc[C + c] += m ? 1.f : 0.f;
        acc[2 * C + c] += m ? q : 0.f;
        if (c == 0) q0 = q;
      }
      const float f = 1.f - q0;
      const bool fg = lab[j] != 0;
      acc[3 * C] += f;
      acc[3 * C + 1] += fg ? 1.f : 0.f;
      acc[3 * C + 2] += fg ? f : 0.f;
      am |= (uint32_t)arg << (8 * j);
    }
    if (lm != nullptr) {
      if constexpr (V == 4) *reinterpret_cast<uint32_t*>(lm + i) = am;
      else lm[i] = (uint8_t)am;
    }
  }
  __shared__ double red[4][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float w = wave_sum(acc[s]);
    if (lane == 0) red[wave][s] = (double)w;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int s = threadIdx.x;
    part[(((long long)b * NS + s) * H + h) * nch + k] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
  }
}

__device__ __forceinline__ double cm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double cm_sigmoid10(double x) { return 1.0 / (1.0 + exp(-(x - 10.0))); }

// out f32 [B + 1][3C + 2].  Row b < B: Dice[C], Recall[C], Precision[C], foreground Dice, LocalizationLoss of sample b.  Row B:
// 1 - mean Dice[C], mean Recall[C], mean Precision[C], 1 - mean foreground Dice, mean LocalizationLoss (the driver's values).
// One workgroup; every sum runs in an order fixed by (B, C, H, nch) alone.  A thread loads all NS statistics of a position
// together, so the fold costs a few memory latencies, not NS of them.
template <int C>
__global__ void __launch_bounds__(256) cm_finalize_kernel(const double* __restrict__ part, float* __restrict__ out, int B, int H,
                                                          int nch) {
  constexpr int NS = 3 * C + 3, NO = 3 * C + 2;
  const long long R = (long long)H * nch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double red[4][NS];
  __shared__ double tot[NS];
  __shared__ double mean[NO];
  __shared__ double wq[2][4], wd[4];
  if (tid < NO) mean[tid] = 0.0;
  const int per = (H + 255) / 256, h0 = tid * per, h1 = min(h0 + per, H);
  for (int b = 0; b < B; ++b) {
    // class / foreground totals over every (row, chunk)
    const double* q = part + (long long)b * NS * R;
    double a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = 0.0;
#pragma unroll 2
    for (long long i = tid; i < R; i += 256) {
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] += q[s * R + i];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const double v = cm_wave_sum(a[s]);
      if (lane == 0) red[wave][s] = v;
    }
    // LocalizationLoss (multi_criterions.py:219-281): the H profiles of 1 - p_0 and [t != 0] through sigmoid(x - 10), their
    // cumulative sums over H normalised by (total + 1e-6), mean over H of the absolute difference.  Thread tid owns rows
    // [h0, h1); an exclusive scan over threads gives each its starting offset.
    const double* fp = part + ((long long)b * NS + 3 * C) * R;
    const double* ft = fp + R;
    double lp = 0.0, lt = 0.0;
    for (int h = h0; h < h1; ++h) {
      double sp = 0.0, st = 0.0;
#pragma unroll 4
      for (int k = 0; k < nch; ++k) { sp += fp[(long long)h * nch + k]; st += ft[(long long)h * nch + k]; }
      lp += cm_sigmoid10(sp);
      lt += cm_sigmoid10(st);
    }
    double ip = lp, it = lt;                                   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(ip, o), ut = __shfl_up(it, o);
      if (lane >= o) { ip += up; it += ut; }
    }
    if (lane == 63) { wq[0][wave] = ip; wq[1][wave] = it; }
    __syncthreads();
    if (tid < NS) tot[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    double cp = __shfl_up(ip, 1), ct = __shfl_up(it, 1);
    if (lane == 0) cp = ct = 0.0;
    double Qp = 0.0, Qt = 0.0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) { cp += wq[0][w]; ct += wq[1][w]; }
      Qp += wq[0][w];
      Qt += wq[1][w];
    }
    double d = 0.0;
    for (int h = h0; h < h1; ++h) {
      double sp = 0.0, st = 0.0;
#pragma unroll 4
      for (int k = 0; k < nch; ++k) { sp += fp[(long long)h * nch + k]; st += ft[(long long)h * nch + k]; }
      cp += cm_sigmoid10(sp);
      ct += cm_sigmoid10(st);
      d += fabs(cp / (Qp + 1e-6) - ct / (Qt + 1e-6));
    }
    d = cm_wave_sum(d);
    if (lane == 0) wd[wave] = d;
    __syncthreads();
    float* o = out + (long long)b * NO;
    if (tid < C) {
      const double sp = tot[tid], st = tot[C + tid], spt = tot[2 * C + tid];
      const double dice = (2.0 * spt + 1e-9) / (sp + st + 1e-9), rec = (spt + 1e-5) / (st + 1e-5), prec = (spt + 1e-5) / (sp + 1e-5);
      o[tid] = (float)dice;
      o[C + tid] = (float)rec;
      o[2 * C + tid] = (float)prec;
      mean[tid] += dice;
      mean[C + tid] += rec;
      mean[2 * C + tid] += prec;
    } else if (tid == C) {
      const double sp = tot[3 * C], st = tot[3 * C + 1], spt = tot[3 * C + 2];
      const double dice = (2.0 * spt + 1e-9) / (sp + st + 1e-9);
      o[3 * C] = (float)dice;
      mean[3 * C] += dice;
    } else if (tid == C + 1) {
      const double loc = (((wd[0] + wd[1]) + wd[2]) + wd[3]) / H;
      o[3 * C + 1] = (float)loc;
      mean[3 * C + 1] += loc;
    }
    __syncthreads();                                          // red / tot / wq / wd are reused by the next sample
  }
  if (tid < NO) {
    const bool dice = tid < C || tid == 3 * C;
    const double m = mean[tid] / B;
    out[(long long)B * NO + tid] = (float)(dice ? 1.0 - m : m);
  }
}

template <int C>
static void cm_launch_stats(bool vec, dim3 grid, hipStream_t st, const float* pred, const uint8_t* target, uint8_t* lmap,
                            double* part, int H, long long WD, long long chunk, float thr) {
  if (vec)
    hipLaunchKernelGGL((cm_stats_kernel<C, 4>), grid, dim3(256), 0, st, pred, target, lmap, part, H, WD, chunk, thr);
  else
    hipLaunchKernelGGL((cm_stats_kernel<C, 1>), grid, dim3(256), 0, st, pred, target, lmap, part, H, WD, chunk, thr);
}

extern "C" long long ltu_class_metrics_ws_elems(int B, int C, int H, int W, int D) {
  if (!cm_shape_ok(B, C, H, W, D)) return 0;
  long long nch, chunk;
  cm_geometry(B, H, (long long)W * D, &nch, &chunk);
  return (long long)B * (3 * C + 3) * H * nch;
}

extern "C" int ltu_class_metrics_pass(const float* pred, const uint8_t* target, uint8_t* label_map, double* scratch,
                                      long long scratch_elems, int B, int C, int H, int W, int D, float threshold, ltu_stream_t s) {
  if (!cm_shape_ok(B, C, H, W, D)) return LTU_E_SHAPE;
  if (threshold != threshold) return LTU_E_ARG;
  if (scratch == nullptr || scratch_elems < ltu_class_metrics_ws_elems(B, C, H, W, D)) return LTU_E_ARG;
  const long long WD = (long long)W * D;
  long long nch, chunk;
  cm_geometry(B, H, WD, &nch, &chunk);
  const bool vec = WD % 4 == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)label_map & 3) == 0;
  const dim3 grid((unsigned)nch, H, B);
  hipStream_t st = (hipStream_t)s;
  switch (C) {
    case 2: cm_launch_stats<2>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
    case 3: cm_launch_stats<3>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
    case 4: cm_launch_stats<4>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
    case 5: cm_launch_stats<5>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
    case 6: cm_launch_stats<6>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
    case 7: cm_launch_stats<7>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
    default: cm_launch_stats<8>(vec, grid, st, pred, target, label_map, scratch, H, WD, chunk, threshold); break;
  }
  return ltu_check_launch();
}

extern "C" int ltu_class_metrics_finalize(const double* scratch, long long scratch_elems, float* out, int B, int C, int H, int W,
                                          int D, ltu_stream_t s) {
  if (!cm_shape_ok(B, C, H, W, D)) return LTU_E_SHAPE;
  if (scratch == nullptr || scratch_elems < ltu_class_metrics_ws_elems(B, C, H, W, D)) return LTU_E_ARG;
  long long nch, chunk;
  cm_geometry(B, H, (long long)W * D, &nch, &chunk);
  hipStream_t st = (hipStream_t)s;
  switch (C) {
    case 2: hipLaunchKernelGGL(cm_finalize_kernel<2>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
    case 3: hipLaunchKernelGGL(cm_finalize_kernel<3>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
    case 4: hipLaunchKernelGGL(cm_finalize_kernel<4>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
    case 5: hipLaunchKernelGGL(cm_finalize_kernel<5>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
    case 6: hipLaunchKernelGGL(cm_finalize_kernel<6>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
    case 7: hipLaunchKernelGGL(cm_finalize_kernel<7>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
    default: hipLaunchKernelGGL(cm_finalize_kernel<8>, dim3(1), dim3(256), 0, st, scratch, out, B, H, (int)nch); break;
  }
  return ltu_check_launch();
}
