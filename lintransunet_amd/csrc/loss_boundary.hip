// Boundary loss of one decoder level (Kervadec et al., "Boundary loss for highly unbalanced segmentation") on the signed distance
// maps of distmap.hip: value_k = (1 / (B S)) sum_b sum_s p[b][s][c_k] phi[b][k][s], total = base + scale sum_k w_k value_k,
// dp[b][s][c_k] = g scale w_k phi[b][k][s] / (B S).  The term rides on a level's existing loss entry (ltu_loss, ltu_loss_wide,
// ltu_loss_ext): the forward adds that entry's total (`base_total`) and the backward adds into the dp it has just written
// (`accumulate`), so no torch arithmetic joins the two.  Per-workgroup partials folded in a fixed order, no atomics.
#include "common.h"

#include <math.h>

#define LB_MAX_K 8
#define LB_THREADS 256
#define LB_MAX_BLOCKS 512         // workgroups per sample of the sums pass

struct LbTerms {
  int cls[LB_MAX_K];              // class of term k
  float w[LB_MAX_K];              // forward: w_k; backward: w_k / (B S)
};

static long long lb_blocks(long long S) {
  long long g = (S + LB_THREADS - 1) / LB_THREADS;
  return g < 1 ? 1 : g > LB_MAX_BLOCKS ? LB_MAX_BLOCKS : g;
}

// part [B gridDim.x][K] doubles: sum over the workgroup's voxels of p[c_k] phi_k.  grid (blocks, B)
__global__ void __launch_bounds__(LB_THREADS) lb_sums_kernel(const float* __restrict__ p, const float* __restrict__ phi,
                                                             double* __restrict__ part, LbTerms t, int K, long long S, int C) {
  __shared__ double red[LB_MAX_K][LB_THREADS];
  const int b = blockIdx.y;
  const float* pb = p + (long long)b * S * C;
  const float* fb = phi + (long long)b * K * S;
  float acc[LB_MAX_K];
#pragma unroll
  for (int k = 0; k < LB_MAX_K; ++k) acc[k] = 0.f;
  for (long long i = (long long)blockIdx.x * LB_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * LB_THREADS) {
#pragma unroll
    for (int k = 0; k < LB_MAX_K; ++k)
      if (k < K) acc[k] = fmaf(pb[i * C + t.cls[k]], fb[(long long)k * S + i], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < LB_MAX_K; ++k) red[k][threadIdx.x] = (double)acc[k];
  __syncthreads();
  for (int o = LB_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if ((int)threadIdx.x < K) part[((long long)b * gridDim.x + blockIdx.x) * K + threadIdx.x] = red[threadIdx.x][0];
}

// fold of the G partials in workgroup order (one lane per term), then the total
__global__ void __launch_bounds__(64) lb_finalize_kernel(const double* __restrict__ part, long long G, LbTerms t, int K, double inv_n,
                                                         float* __restrict__ values, const float* __restrict__ base_total,
                                                         const float* __restrict__ scale_dev, const float* __restrict__ term_scale_dev) {
  __shared__ float val[LB_MAX_K];
  if ((int)threadIdx.x < K) {
    double acc = 0.0;
    for (long long g = 0; g < G; ++g) acc += part[g * K + threadIdx.x];
    const float v = (float)(acc * inv_n);
    val[threadIdx.x] = v;
    values[1 + threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float scale = (scale_dev ? scale_dev[0] : 1.f) * (term_scale_dev ? term_scale_dev[0] : 1.f);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum = fmaf(t.w[k], val[k], sum);
    values[0] = (base_total ? base_total[0] : 0.f) + scale * sum;
  }
}

// one thread per voxel: its C channels of dp.  t.w[k] = w_k / (B S)
template <int CT, bool ACC>
__global__ void __launch_bounds__(LB_THREADS) lb_bwd_kernel(const float* __restrict__ phi, float* __restrict__ dp, LbTerms t, int K,
                                                            long long S, const float* __restrict__ scale_dev,
                                                            const float* __restrict__ term_scale_dev, const float* __restrict__ gscale) {
  const int b = blockIdx.y;
  const float gs = gscale[0] * ((scale_dev ? scale_dev[0] : 1.f) * (term_scale_dev ? term_scale_dev[0] : 1.f));
  const float* fb = phi + (long long)b * K * S;
  float* db = dp + (long long)b * S * CT;
  for (long long i = (long long)blockIdx.x * LB_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * LB_THREADS) {
    float d[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) d[c] = ACC ? db[i * CT + c] : 0.f;
#pragma unroll
    for (int k = 0; k < LB_MAX_K; ++k) {
      if (k < K) {
        const float v = (gs * t.w[k]) * fb[(long long)k * S + i];
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (t.cls[k] == c) d[c] += v;
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) db[i * CT + c] = d[c];
  }
}

static int lb_check(const int* classes, const float* w, int K, int B, long long S, int C, LbTerms* t) {
  if (B <= 0 || B > 65535 || S <= 0 || C < 2 || C > LTU_WIDE_MAXC || K < 1 || K > LB_MAX_K) return LTU_E_SHAPE;
  if (classes == nullptr || w == nullptr) return LTU_E_ARG;
  for (int k = 0; k < LB_MAX_K; ++k) { t->cls[k] = 0; t->w[k] = 0.f; }
  for (int k = 0; k < K; ++k) {
    if (classes[k] < 0 || classes[k] >= C || !isfinite(w[k])) return LTU_E_ARG;
    t->cls[k] = classes[k];
    t->w[k] = w[k];
  }
  return LTU_OK;
}

extern "C" long long ltu_loss_boundary_sums_floats(int B, long long S, int K) {
  if (B <= 0 || S <= 0 || K <= 0) return 0;
  return 2LL * B * lb_blocks(S) * K;            // doubles, counted in floats
}

extern "C" int ltu_loss_boundary_fwd(const float* p, const float* phi, const int* classes, const float* w, int K, float* sums,
                                     long long sums_floats, float* values, const float* base_total, const float* scale_dev,
                                     const float* term_scale_dev, int B, long long S, int C, ltu_stream_t s) {
  LbTerms t;
  const int rc = lb_check(classes, w, K, B, S, C, &t);
  if (rc != LTU_OK) return rc;
  if (p == nullptr || phi == nullptr || sums == nullptr || values == nullptr) return LTU_E_ARG;
  if (sums_floats < ltu_loss_boundary_sums_floats(B, S, K) || ((uintptr_t)sums & 7)) return LTU_E_ARG;
  const long long gx = lb_blocks(S);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(lb_sums_kernel, dim3((unsigned)gx, B), dim3(LB_THREADS), 0, st, p, phi, (double*)sums, t, K, S, C);
  hipLaunchKernelGGL(lb_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)sums, gx * B, t, K, 1.0 / ((double)B * (double)S),
                     values, base_total, scale_dev, term_scale_dev);
  return ltu_check_launch();
}

extern "C" int ltu_loss_boundary_bwd(const float* phi, const int* classes, const float* w, int K, const float* scale_dev,
                                     const float* term_scale_dev, const float* gscale, float* dp, int accumulate, int B, long long S,
                                     int C, ltu_stream_t s) {
  LbTerms t;
  const int rc = lb_check(classes, w, K, B, S, C, &t);
  if (rc != LTU_OK) return rc;
  if (phi == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  for (int k = 0; k < K; ++k) t.w[k] = (float)((double)w[k] / ((double)B * (double)S));
  long long gx = (S + LB_THREADS - 1) / LB_THREADS;
  if (gx > 4096) gx = 4096;
  hipStream_t st = (hipStream_t)s;
  LTU_DISPATCH_C(C, {
    if (accumulate)
      hipLaunchKernelGGL((lb_bwd_kernel<CT, true>), dim3((unsigned)gx, B), dim3(LB_THREADS), 0, st, phi, dp, t, K, S, scale_dev,
                         term_scale_dev, gscale);
    else
      hipLaunchKernelGGL((lb_bwd_kernel<CT, false>), dim3((unsigned)gx, B), dim3(LB_THREADS), 0, st, phi, dp, t, K, S, scale_dev,
                         term_scale_dev, gscale);
  });
  return ltu_check_launch();
}
