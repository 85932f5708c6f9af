// Soft morphology on fp32 volumes [N][H][W][D], the soft skeleton built from it, the skeleton of 0 / 1 label maps on bytes, and
// soft-clDice (Shit et al., CVPR 2021) as the fifth stage of a level's loss chain.
//
//   erode(x)[v]  = min over the 7-voxel cross {centre, -H, +H, -W, +W, -D, +D}           (the minimum of three 1-D 3-pools)
//   dilate(x)[v] = max over the 3 x 3 x 3 cube
// Taps outside the volume are left out (a max-pool padded with -inf); an axis of extent 1 has no neighbours.  The tap of an output
// voxel is the FIRST that attains the extremum in the order: centre, then for erode -H, +H, -W, +W, -D, +D (codes 0 .. 6), for
// dilate the other 26 in raster order of (dh, dw, dd), dd fastest (codes r = 9 (dh + 1) + 3 (dw + 1) + (dd + 1), centre 13).  A
// later tap replaces the running extremum only where it is strictly smaller (larger), so on a plateau the gradient stays at the
// centre.  The forward stores the tap code, one byte per voxel and operator.
//   skeleton: I_0 = x, I_{j+1} = erode(I_j), D_j = dilate(I_{j+1}), delta_j = relu(I_j - D_j),
//             s_0 = delta_0, s_j = s_{j-1} + relu(delta_j - s_{j-1} delta_j), result s_iters; relu'(0) = 0.
// Evaluation order.  This file is compiled with -ffp-contract=off (csrc/Makefile): a product meets a sum in one rounding only where
// fmaf is written, which is in two places, both named below.  delta_j - s_{j-1} delta_j is a product rounded on its own and a rounded
// difference, then one rounded add onto s_{j-1}, as an fp32 evaluation op by op gives it.  The backward is a gather and evaluates,
// per voxel v and with r_j = [I_j > D_j], m_j = [delta_j - s_{j-1} delta_j > 0], g the gradient of s_iters:
//     for j = iters .. 1:  e_j = r_j m_j (g - g s_{j-1});   g = m_j ? g - g delta_j : g         (products rounded on their own)
//     e_0 = r_0 g
// (the point pass; I_j[v] and D_j[v] = I_{j+1}[v + tap] are re-read and s_j re-formed with the forward's instructions), then for
// k = iters + 1 .. 0 the gradient of I_k, each voxel u collecting in this order with plain rounded adds:
//     G_k[u] = e_k[u]   (k <= iters)
//            - e_{k-1}[v] for the 27 cube neighbours v of u in raster order whose dilate tap is u       (k >= 1)
//            + G_{k+1}[v] for v = u, u-H, u+H, u-W, u+W, u-D, u+D whose erode tap is u                  (k <= iters)
// G_0 is the gradient of x.  No atomics of any kind: two calls agree bit for bit.
//
// clDice stage, for term k of class c = classes[k], P = p[..., c], G = [label == c], S_P = skeleton(P), S_G the label skeleton, sums
// over the whole batch taken in double (per-thread, per-workgroup tree, then a fold of the workgroups' partials in index order):
//     Tprec = (sum S_P G + 1) / (sum S_P + 1)     Tsens = (sum S_G P + 1) / (sum S_G + 1)     value = 1 - 2 Tprec Tsens / (Tprec + Tsens)
// formed in double by one thread and rounded once; total = base + scale sum_k w_k value_k, the terms added in k order with fmaf in
// fp32.  The seed of the skeleton's backward is gscale (a G + b), a = q / (sum S_P + 1), b = -q Tprec / (sum S_P + 1), q = scale w_k
// dvalue/dTprec, evaluated as fmaf(a, G, b) times gscale; the direct gradient into P is gscale c S_G, c = scale w_k dvalue/dTsens /
// (sum S_G + 1), formed as (gscale c) S_G, two rounded products, and added to G_0 last with a rounded add.  The two fmaf of the file:
// the seed's fmaf(a, G, b) and the total's fmaf(scale w_k, value_k, total).
#include "common.h"

#include <math.h>

#define SM_MAX_ITERS 10
#define SM_MAX_K 8
#define SM_SUM_CHUNK 4096      // voxels per workgroup of the stage's sums pass: 16 per thread

// where level 0 of a chain lives: volume n, voxel s is x[(n / K) bstride + s estride + cls[n % K]].  A contiguous [N][S] array is
// K = 1, bstride = S, estride = 1; channel cls[k] of channels-last probabilities [B][S][C] is bstride = S C, estride = C.
struct SmSrc {
  const float* x;
  long long bstride;
  int estride, K;
  int cls[SM_MAX_K];
};

struct SmDim {
  int H, W, D;
  long long S, NS;      // H W D, N H W D
};

__device__ __forceinline__ const float* sm_base(const SmSrc& src, long long n) {
  const long long b = n / src.K;
  const int k = (int)(n - b * src.K);
  int c = 0;
#pragma unroll
  for (int q = 0; q < SM_MAX_K; ++q) c = k == q ? src.cls[q] : c;
  return src.x + b * src.bstride + c;
}

// flat index -> volume, voxel and coordinates; false past the end
__device__ __forceinline__ bool sm_decode(const SmDim& g, long long& idx, long long& n, int& s, int& h, int& w, int& d) {
  idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= g.NS) return false;
  n = idx / g.S;
  s = (int)(idx - n * g.S);
  d = s % g.D;
  const int hw = s / g.D;
  w = hw % g.W;
  h = hw / g.W;
  return true;
}

__device__ __forceinline__ float sm_relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ forward
__global__ void __launch_bounds__(256) sm_erode_kernel(SmSrc in, float* __restrict__ out, uint8_t* __restrict__ tap, SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  const float* x = sm_base(in, n);
  const long long es = in.estride;
  const int WD = g.W * g.D;
  float m = x[s * es];
  int t = 0;
  float v;
  if (h > 0) { v = x[(s - WD) * es]; if (v < m) { m = v; t = 1; } }
  if (h + 1 < g.H) { v = x[(s + WD) * es]; if (v < m) { m = v; t = 2; } }
  if (w > 0) { v = x[(s - g.D) * es]; if (v < m) { m = v; t = 3; } }
  if (w + 1 < g.W) { v = x[(s + g.D) * es]; if (v < m) { m = v; t = 4; } }
  if (d > 0) { v = x[(s - 1) * es]; if (v < m) { m = v; t = 5; } }
  if (d + 1 < g.D) { v = x[(s + 1) * es]; if (v < m) { m = v; t = 6; } }
  out[idx] = m;
  tap[idx] = (uint8_t)t;
}

// the maximum of x over the cube at (h, w, d) of one contiguous volume and its tap code
__device__ __forceinline__ float sm_cube_max(const float* __restrict__ x, int s, int h, int w, int d, const SmDim& g, int& tap) {
  const int WD = g.W * g.D;
  float m = x[s];
  int t = 13;
#pragma unroll
  for (int dh = -1; dh <= 1; ++dh) {
#pragma unroll
    for (int dw = -1; dw <= 1; ++dw) {
#pragma unroll
      for (int dd = -1; dd <= 1; ++dd) {
        if (dh == 0 && dw == 0 && dd == 0) continue;
        if (h + dh < 0 || h + dh >= g.H || w + dw < 0 || w + dw >= g.W || d + dd < 0 || d + dd >= g.D) continue;
        const float v = x[s + dh * WD + dw * g.D + dd];
        if (v > m) { m = v; t = 9 * (dh + 1) + 3 * (dw + 1) + (dd + 1); }
      }
    }
  }
  tap = t;
  return m;
}

// UPDATE false: out = dilate(nxt).  UPDATE true, one skeleton iteration: D_j = dilate(nxt = I_{j+1}), delta_j = relu(I_j - D_j) with
// I_j = cur, and sk holds s_{j-1} on entry (not read when first) and s_j on exit
template <bool UPDATE>
__global__ void __launch_bounds__(256) sm_dilate_kernel(SmSrc cur, const float* __restrict__ nxt, uint8_t* __restrict__ tap, float* __restrict__ out,
                                                        int first, SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  int t;
  const float m = sm_cube_max(nxt + n * g.S, s, h, w, d, g, t);
  tap[idx] = (uint8_t)t;
  if constexpr (!UPDATE) {
    out[idx] = m;
  } else {
    const float delta = sm_relu(sm_base(cur, n)[(long long)s * cur.estride] - m);
    float sk = delta;
    if (!first) {
      const float prev = out[idx];
      sk = (prev + sm_relu((delta - (prev * delta))));
    }
    out[idx] = sk;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// what seeds the skeleton's backward in the clDice stage: gscale (a G + b) per voxel (gout of the point pass is null then)
struct SmSeed {
  const uint8_t* label;        // [B][S]
  const float* coef;           // [K][3] = (a, b, c)
  const float* gscale;
};

// The point pass: e_j[v] for j = 0 .. iters.  I holds I_1 .. I_{iters+1}, tapD the dilate taps of D_0 .. D_iters, E receives e_0 ..
__global__ void __launch_bounds__(256) sm_bwd_point_kernel(SmSrc x0, const float* __restrict__ I, const uint8_t* __restrict__ tapD,
                                                           const float* __restrict__ gout, SmSeed seed, float* __restrict__ E, int iters, SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  const int WD = g.W * g.D;
  float diff[SM_MAX_ITERS + 1], sk[SM_MAX_ITERS + 1], u[SM_MAX_ITERS + 1];
  float prev = sm_base(x0, n)[(long long)s * x0.estride];
#pragma unroll
  for (int j = 0; j <= SM_MAX_ITERS; ++j) {
    diff[j] = 0.f; sk[j] = 0.f; u[j] = 0.f;
    if (j <= iters) {
      const float* nx = I + (long long)j * g.NS;
      int t = tapD[(long long)j * g.NS + idx];
      int dh = t / 9 - 1, dw = (t / 3) % 3 - 1, dd = t % 3 - 1;
      if (t > 26 || h + dh < 0 || h + dh >= g.H || w + dw < 0 || w + dw >= g.W || d + dd < 0 || d + dd >= g.D) { dh = 0; dw = 0; dd = 0; }
      diff[j] = prev - nx[idx + dh * WD + dw * g.D + dd];
      const float delta = sm_relu(diff[j]);
      if (j == 0) sk[0] = delta;
      else {
        u[j] = (delta - (sk[j - 1] * delta));
        sk[j] = (sk[j - 1] + sm_relu(u[j]));
      }
      prev = nx[idx];
    }
  }
  float gs;
  if (gout) gs = gout[idx];
  else {
    const long long b = n / x0.K;
    const int k = (int)(n - b * x0.K);
    int c = 0;
#pragma unroll
    for (int q = 0; q < SM_MAX_K; ++q) c = k == q ? x0.cls[q] : c;
    const float G = seed.label[b * g.S + s] == c ? 1.f : 0.f;
    gs = seed.gscale[0] * fmaf(seed.coef[k * 3], G, seed.coef[k * 3 + 1]);
  }
#pragma unroll
  for (int j = SM_MAX_ITERS; j >= 1; --j) {
    if (j <= iters) {
      const bool m = u[j] > 0.f;
      const float delta = sm_relu(diff[j]);
      E[(long long)j * g.NS + idx] = (m && diff[j] > 0.f) ? (gs - (gs * sk[j - 1])) : 0.f;
      gs = m ? (gs - (gs * delta)) : gs;
    }
  }
  E[idx] = diff[0] > 0.f ? gs : 0.f;
}

// where G_0 goes: a contiguous dx, or channel cls[k] of dp [B][S][C] with the stage's direct term c S_G added last
struct SmOut {
  float* out;
  long long bstride;
  int estride, K;
  int cls[SM_MAX_K];
  const uint8_t* skel;         // [N][S] label skeleton (null: no direct term)
  const float* coef;           // [K][3]
  const float* gscale;
  int accumulate;              // add into what out holds
};

// The gather of level k (file header).  Ek, Ekm1 (with tapD of D_{k-1}) and Gnext (with tapE of I_{k+1}) may each be null; dsign is
// the sign with which Ekm1 enters (-1 in the skeleton, +1 for the dilate operator alone)
__global__ void __launch_bounds__(256) sm_bwd_gather_kernel(const float* __restrict__ Ek, const float* __restrict__ Ekm1, const uint8_t* __restrict__ tapD,
                                                            float dsign, const float* __restrict__ Gnext, const uint8_t* __restrict__ tapE, SmOut o,
                                                            SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  const int WD = g.W * g.D;
  float acc = Ek ? Ek[idx] : 0.f;
  if (Ekm1) {
#pragma unroll
    for (int dh = -1; dh <= 1; ++dh) {
#pragma unroll
      for (int dw = -1; dw <= 1; ++dw) {
#pragma unroll
        for (int dd = -1; dd <= 1; ++dd) {
          if (h + dh < 0 || h + dh >= g.H || w + dw < 0 || w + dw >= g.W || d + dd < 0 || d + dd >= g.D) continue;
          const long long v = idx + dh * WD + dw * g.D + dd;
          const int r = 9 * (dh + 1) + 3 * (dw + 1) + (dd + 1);
          if (tapD[v] == 26 - r) acc = (acc + dsign * Ekm1[v]);
        }
      }
    }
  }
  if (Gnext) {
    if (tapE[idx] == 0) acc = (acc + Gnext[idx]);
    if (h > 0 && tapE[idx - WD] == 2) acc = (acc + Gnext[idx - WD]);
    if (h + 1 < g.H && tapE[idx + WD] == 1) acc = (acc + Gnext[idx + WD]);
    if (w > 0 && tapE[idx - g.D] == 4) acc = (acc + Gnext[idx - g.D]);
    if (w + 1 < g.W && tapE[idx + g.D] == 3) acc = (acc + Gnext[idx + g.D]);
    if (d > 0 && tapE[idx - 1] == 6) acc = (acc + Gnext[idx - 1]);
    if (d + 1 < g.D && tapE[idx + 1] == 5) acc = (acc + Gnext[idx + 1]);
  }
  const long long b = n / o.K;
  const int k = (int)(n - b * o.K);
  int c = 0;
#pragma unroll
  for (int q = 0; q < SM_MAX_K; ++q) c = k == q ? o.cls[q] : c;
  if (o.skel) acc = (acc + ((o.gscale[0] * o.coef[k * 3 + 2]) * (float)o.skel[idx]));
  float* dst = o.out + b * o.bstride + (long long)s * o.estride + c;
  *dst = o.accumulate ? (*dst + acc) : acc;
}

// ------------------------------------------------------------------------------------------------ label skeleton on bytes
// On a 0 / 1 volume every value of the chain stays in {0, 1}: erode is AND over the cross, dilate OR over the cube, delta = I and not
// D, s = s or delta.  The result's own bytes carry the state between launches: bit 0 = s, bits 1 and 2 = I_j and I_{j+1}, swapping
// roles each iteration.  A launch writes one bit of a thread's own byte and reads from its neighbours only a bit that no thread
// changes in that launch (relaxed byte loads and stores), so no second volume is needed.
__device__ __forceinline__ int sm_ldb(const uint8_t* a) { return (int)__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sm_stb(uint8_t* a, int v) { __hip_atomic_store(a, (uint8_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct SmCls { int K; int cls[SM_MAX_K]; };

// out byte = I_0 (bit 1) | I_1 (bit 2), straight from the label: no thread reads `out` here.  out [B][K][S], NS = B K S
__global__ void __launch_bounds__(256) sm_label_init_kernel(const uint8_t* __restrict__ label, SmCls cc, uint8_t* __restrict__ out, SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  const long long b = n / cc.K;
  const int k = (int)(n - b * cc.K);
  int c = 0;
#pragma unroll
  for (int q = 0; q < SM_MAX_K; ++q) c = k == q ? cc.cls[q] : c;
  const uint8_t* x = label + b * g.S;
  const int WD = g.W * g.D;
  const int i0 = x[s] == c;
  int e = i0;
  if (h > 0) e &= x[s - WD] == c;
  if (h + 1 < g.H) e &= x[s + WD] == c;
  if (w > 0) e &= x[s - g.D] == c;
  if (w + 1 < g.W) e &= x[s + g.D] == c;
  if (d > 0) e &= x[s - 1] == c;
  if (d + 1 < g.D) e &= x[s + 1] == c;
  out[idx] = (uint8_t)((i0 << 1) | (e << 2));
}

// bit `to` of the own byte = AND over the cross of bit `from`
__global__ void __launch_bounds__(256) sm_label_erode_kernel(uint8_t* out, int from, int to, SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  const int WD = g.W * g.D;
  const int own = sm_ldb(out + idx);
  int e = own;
  if (h > 0) e &= sm_ldb(out + idx - WD);
  if (h + 1 < g.H) e &= sm_ldb(out + idx + WD);
  if (w > 0) e &= sm_ldb(out + idx - g.D);
  if (w + 1 < g.W) e &= sm_ldb(out + idx + g.D);
  if (d > 0) e &= sm_ldb(out + idx - 1);
  if (d + 1 < g.D) e &= sm_ldb(out + idx + 1);
  sm_stb(out + idx, (own & ~(1 << to)) | (((e >> from) & 1) << to));
}

// bit 0 of the own byte |= I_j and not OR over the cube of I_{j+1}; bit `cur` = I_j, bit `nxt` = I_{j+1}
__global__ void __launch_bounds__(256) sm_label_update_kernel(uint8_t* out, int cur, int nxt, SmDim g) {
  long long idx, n; int s, h, w, d;
  if (!sm_decode(g, idx, n, s, h, w, d)) return;
  const int WD = g.W * g.D;
  const int own = sm_ldb(out + idx);
  int m = 0;
#pragma unroll
  for (int dh = -1; dh <= 1; ++dh) {
#pragma unroll
    for (int dw = -1; dw <= 1; ++dw) {
#pragma unroll
      for (int dd = -1; dd <= 1; ++dd) {
        if (h + dh < 0 || h + dh >= g.H || w + dw < 0 || w + dw >= g.W || d + dd < 0 || d + dd >= g.D) continue;
        m |= sm_ldb(out + idx + dh * WD + dw * g.D + dd);
      }
    }
  }
  const int delta = ((own >> cur) & 1) & ~((m >> nxt) & 1);
  sm_stb(out + idx, own | delta);
}

__global__ void __launch_bounds__(256) sm_label_final_kernel(uint8_t* __restrict__ out, long long NS) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx < NS) out[idx] &= 1;
}

// ------------------------------------------------------------------------------------------------ the clDice stage
// Workgroup (x, k): voxels [x SM_SUM_CHUNK, ..) of the batch's B S, term k.  part [gridDim.x][K][4] = {sum S_P G, sum S_P, sum S_G P,
// sum S_G} in double; S_G is copied to `keep` for the backward
__global__ void __launch_bounds__(256) cld_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, const uint8_t* __restrict__ skel,
                                                       const float* __restrict__ sp, SmCls cc, double* __restrict__ part, uint8_t* __restrict__ keep,
                                                       long long S, long long BS, int C) {
  __shared__ double red[4][256];
  const int k = blockIdx.y;
  int c = 0;
#pragma unroll
  for (int q = 0; q < SM_MAX_K; ++q) c = k == q ? cc.cls[q] : c;
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
  const long long i0 = (long long)blockIdx.x * SM_SUM_CHUNK;
  for (int t = 0; t < SM_SUM_CHUNK / 256; ++t) {
    const long long i = i0 + t * 256 + threadIdx.x;
    if (i < BS) {
      const long long b = i / S;
      const long long v = (b * cc.K + k) * S + (i - b * S);
      const float s_p = sp[v];
      const uint8_t s_g = skel[v];
      keep[v] = s_g;
      a0 += label[i] == c ? (double)s_p : 0.;
      a1 += (double)s_p;
      a2 += s_g ? (double)p[i * C + c] : 0.;
      a3 += s_g ? 1. : 0.;
    }
  }
  red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1; red[2][threadIdx.x] = a2; red[3][threadIdx.x] = a3;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) part[((long long)blockIdx.x * cc.K + k) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

struct CldCfg { int K; float w[SM_MAX_K]; };

// One workgroup: the partials of each (k, sum) folded by 256 threads striding the workgroups and a tree, then thread 0 forms the
// values [total, value_0 ..] and coef [K][3] = (a, b, c)
__global__ void __launch_bounds__(256) cld_finalize_kernel(const double* __restrict__ part, int nblk, CldCfg cfg, float* __restrict__ values,
                                                           float* __restrict__ coef, const float* __restrict__ base_total, const float* __restrict__ scale_dev) {
  __shared__ double red[256];
  __shared__ double sums[SM_MAX_K * 4];
  for (int q = 0; q < cfg.K * 4; ++q) {
    double a = 0.;
    for (int i = threadIdx.x; i < nblk; i += 256) a += part[(long long)i * cfg.K * 4 + q];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[q] = red[0];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float sc = scale_dev ? scale_dev[0] : 1.f;
  float total = base_total ? base_total[0] : 0.f;
#pragma unroll
  for (int k = 0; k < SM_MAX_K; ++k) {
    if (k < cfg.K) {
      const double A = sums[k * 4], Bs = sums[k * 4 + 1], Cc = sums[k * 4 + 2], Dd = sums[k * 4 + 3];
      const double tp = (A + 1.) / (Bs + 1.), ts = (Cc + 1.) / (Dd + 1.);
      const double den = tp + ts;
      const float value = (float)(1. - 2. * tp * ts / den);
      const double wk = (double)sc * (double)cfg.w[k];
      const double dtp = -2. * ts * ts / (den * den), dts = -2. * tp * tp / (den * den);
      coef[k * 3] = (float)(wk * dtp / (Bs + 1.));
      coef[k * 3 + 1] = (float)(-wk * dtp * tp / (Bs + 1.));
      coef[k * 3 + 2] = (float)(wk * dts / (Dd + 1.));
      values[1 + k] = value;
      total = fmaf(sc * cfg.w[k], value, total);
    }
  }
  values[0] = total;
}

// ------------------------------------------------------------------------------------------------ host side
static bool sm_dims_ok(long long N, int H, int W, int D) {
  if (N < 1 || H < 1 || W < 1 || D < 1) return false;
  const long long S = (long long)H * W * D;
  return S < (1ll << 31) && N <= (1ll << 38) / S;      // voxel offsets fit an int, the flat index and the grid a long long / an int
}
static SmDim sm_dim(long long N, int H, int W, int D) {
  SmDim g;
  g.H = H; g.W = W; g.D = D;
  g.S = (long long)H * W * D;
  g.NS = N * g.S;
  return g;
}
static SmSrc sm_plain(const float* x, long long S) {
  SmSrc r;
  r.x = x; r.bstride = S; r.estride = 1; r.K = 1;
  for (int q = 0; q < SM_MAX_K; ++q) r.cls[q] = 0;
  return r;
}

// the skeleton's scratch in 4-byte elements: I_1 .. I_L and e_0 .. e_{L-1} (L = iters + 1), G ping and pong, then the 2 L tap bytes
struct SmWs {
  float *I, *E, *G0, *G1;
  uint8_t *tapE, *tapD;
  long long elems;
};
static SmWs sm_ws(void* scratch, long long NS, int iters) {
  const long long L = iters + 1;
  SmWs w;
  w.I = (float*)scratch;
  w.E = w.I + L * NS;
  w.G0 = w.E + L * NS;
  w.G1 = w.G0 + NS;
  w.tapE = (uint8_t*)(w.G1 + NS);
  w.tapD = w.tapE + L * NS;
  w.elems = (2 * L + 2) * NS + (2 * L * NS + 3) / 4;
  return w;
}

static void sm_skeleton_fwd(const SmSrc& src, float* sk, const SmWs& ws, const SmDim& g, int iters, hipStream_t st) {
  const dim3 grid(cdiv(g.NS, 256)), block(256);
  for (int j = 0; j <= iters; ++j) {
    const SmSrc cur = j == 0 ? src : sm_plain(ws.I + (long long)(j - 1) * g.NS, g.S);
    float* nxt = ws.I + (long long)j * g.NS;
    hipLaunchKernelGGL(sm_erode_kernel, grid, block, 0, st, cur, nxt, ws.tapE + (long long)j * g.NS, g);
    hipLaunchKernelGGL((sm_dilate_kernel<true>), grid, block, 0, st, cur, (const float*)nxt, ws.tapD + (long long)j * g.NS, sk, (int)(j == 0), g);
  }
}

static void sm_skeleton_bwd(const SmSrc& src, const float* gout, const SmSeed& seed, const SmOut& out, const SmWs& ws, const SmDim& g, int iters,
                            hipStream_t st) {
  const dim3 grid(cdiv(g.NS, 256)), block(256);
  const int L = iters + 1;
  hipLaunchKernelGGL(sm_bwd_point_kernel, grid, block, 0, st, src, (const float*)ws.I, (const uint8_t*)ws.tapD, gout, seed, ws.E, iters, g);
  SmOut mid;
  mid.bstride = g.S; mid.estride = 1; mid.K = 1;
  for (int q = 0; q < SM_MAX_K; ++q) mid.cls[q] = 0;
  mid.skel = nullptr; mid.coef = nullptr; mid.gscale = nullptr; mid.accumulate = 0;
  for (int k = L; k >= 0; --k) {
    const float* Ek = k < L ? ws.E + (long long)k * g.NS : nullptr;
    const float* Ekm1 = k > 0 ? ws.E + (long long)(k - 1) * g.NS : nullptr;
    const uint8_t* tD = k > 0 ? ws.tapD + (long long)(k - 1) * g.NS : nullptr;
    const float* Gn = k < L ? (((k + 1) & 1) ? ws.G1 : ws.G0) : nullptr;
    const uint8_t* tE = k < L ? ws.tapE + (long long)k * g.NS : nullptr;
    mid.out = (k & 1) ? ws.G1 : ws.G0;
    hipLaunchKernelGGL(sm_bwd_gather_kernel, grid, block, 0, st, Ek, Ekm1, tD, -1.f, Gn, tE, k > 0 ? mid : out, g);
  }
}

extern "C" long long ltu_soft_skeleton_scratch_elems(long long N, int H, int W, int D, int iters) {
  if (!sm_dims_ok(N, H, W, D) || iters < 1 || iters > SM_MAX_ITERS) return 0;
  return sm_ws(nullptr, N * (long long)H * W * D, iters).elems;
}

extern "C" int ltu_soft_morph_fwd(const float* x, float* y, uint8_t* tap, int op, long long N, int H, int W, int D, ltu_stream_t s) {
  if (!sm_dims_ok(N, H, W, D)) return LTU_E_SHAPE;
  if (x == nullptr || y == nullptr || tap == nullptr || (op != 0 && op != 1)) return LTU_E_ARG;
  const SmDim g = sm_dim(N, H, W, D);
  const dim3 grid(cdiv(g.NS, 256)), block(256);
  hipStream_t st = (hipStream_t)s;
  if (op == 0) hipLaunchKernelGGL(sm_erode_kernel, grid, block, 0, st, sm_plain(x, g.S), y, tap, g);
  else hipLaunchKernelGGL((sm_dilate_kernel<false>), grid, block, 0, st, sm_plain(x, g.S), x, tap, y, 0, g);
  return ltu_check_launch();
}

extern "C" int ltu_soft_morph_bwd(const float* g_out, const uint8_t* tap, float* dx, int op, long long N, int H, int W, int D, ltu_stream_t s) {
  if (!sm_dims_ok(N, H, W, D)) return LTU_E_SHAPE;
  if (g_out == nullptr || dx == nullptr || tap == nullptr || (op != 0 && op != 1)) return LTU_E_ARG;
  const SmDim g = sm_dim(N, H, W, D);
  const dim3 grid(cdiv(g.NS, 256)), block(256);
  SmOut o;
  o.out = dx; o.bstride = g.S; o.estride = 1; o.K = 1;
  for (int q = 0; q < SM_MAX_K; ++q) o.cls[q] = 0;
  o.skel = nullptr; o.coef = nullptr; o.gscale = nullptr; o.accumulate = 0;
  const float* none = nullptr;
  const uint8_t* notap = nullptr;
  hipStream_t st = (hipStream_t)s;
  if (op == 0) hipLaunchKernelGGL(sm_bwd_gather_kernel, grid, block, 0, st, none, none, notap, 1.f, g_out, tap, o, g);
  else hipLaunchKernelGGL(sm_bwd_gather_kernel, grid, block, 0, st, none, g_out, tap, 1.f, none, notap, o, g);
  return ltu_check_launch();
}

extern "C" int ltu_soft_skeleton_fwd(const float* x, float* y, void* scratch, long long scratch_elems, long long N, int H, int W, int D,
                                     int iters, ltu_stream_t s) {
  if (!sm_dims_ok(N, H, W, D)) return LTU_E_SHAPE;
  if (x == nullptr || y == nullptr || scratch == nullptr || iters < 1 || iters > SM_MAX_ITERS) return LTU_E_ARG;
  const SmDim g = sm_dim(N, H, W, D);
  const SmWs ws = sm_ws(scratch, g.NS, iters);
  if (scratch_elems < ws.elems) return LTU_E_ARG;
  sm_skeleton_fwd(sm_plain(x, g.S), y, ws, g, iters, (hipStream_t)s);
  return ltu_check_launch();
}

extern "C" int ltu_soft_skeleton_bwd(const float* x, const float* g_out, float* dx, void* scratch, long long scratch_elems, long long N,
                                     int H, int W, int D, int iters, ltu_stream_t s) {
  if (!sm_dims_ok(N, H, W, D)) return LTU_E_SHAPE;
  if (x == nullptr || g_out == nullptr || dx == nullptr || scratch == nullptr || iters < 1 || iters > SM_MAX_ITERS) return LTU_E_ARG;
  const SmDim g = sm_dim(N, H, W, D);
  const SmWs ws = sm_ws(scratch, g.NS, iters);
  if (scratch_elems < ws.elems) return LTU_E_ARG;
  SmOut o;
  o.out = dx; o.bstride = g.S; o.estride = 1; o.K = 1;
  for (int q = 0; q < SM_MAX_K; ++q) o.cls[q] = 0;
  o.skel = nullptr; o.coef = nullptr; o.gscale = nullptr; o.accumulate = 0;
  SmSeed seed;
  seed.label = nullptr; seed.coef = nullptr; seed.gscale = nullptr;
  sm_skeleton_bwd(sm_plain(x, g.S), g_out, seed, o, ws, g, iters, (hipStream_t)s);
  return ltu_check_launch();
}

static bool sm_classes_ok(const int* classes, int K, int C) {
  if (classes == nullptr || K < 1 || K > SM_MAX_K) return false;
  for (int k = 0; k < K; ++k) {
    if (classes[k] < 0 || classes[k] >= C) return false;
    for (int q = 0; q < k; ++q)
      if (classes[q] == classes[k]) return false;
  }
  return true;
}

extern "C" int ltu_label_skeletons(const uint8_t* label, const int* classes, int K, uint8_t* out, int B, int H, int W, int D, int iters,
                                   ltu_stream_t s) {
  if (K < 1 || K > SM_MAX_K || !sm_dims_ok((long long)(B > 0 ? B : 0) * K, H, W, D)) return LTU_E_SHAPE;
  if (label == nullptr || out == nullptr || !sm_classes_ok(classes, K, 256) || iters < 1 || iters > SM_MAX_ITERS) return LTU_E_ARG;
  const SmDim g = sm_dim((long long)B * K, H, W, D);
  const dim3 grid(cdiv(g.NS, 256)), block(256);
  SmCls cc;
  cc.K = K;
  for (int q = 0; q < SM_MAX_K; ++q) cc.cls[q] = q < K ? classes[q] : 0;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(sm_label_init_kernel, grid, block, 0, st, label, cc, out, g);
  int cur = 1, nxt = 2;
  for (int j = 0; j <= iters; ++j) {
    if (j > 0) hipLaunchKernelGGL(sm_label_erode_kernel, grid, block, 0, st, out, cur, nxt, g);
    hipLaunchKernelGGL(sm_label_update_kernel, grid, block, 0, st, out, cur, nxt, g);
    const int t = cur; cur = nxt; nxt = t;
  }
  hipLaunchKernelGGL(sm_label_final_kernel, grid, block, 0, st, out, g.NS);
  return ltu_check_launch();
}

// the stage's scratch in 4-byte elements: the partials and sums in double [nblk][K][4], coef [K][3] (32 floats), S_P [B K][S], the
// skeleton's scratch, then the copy of S_G in bytes
struct CldWs {
  double* part;
  float *coef, *sp;
  void* skel_ws;
  uint8_t* keep;
  int nblk;
  long long elems;
};
static CldWs cld_ws(void* scratch, int B, long long S, int K, int iters) {
  CldWs w;
  const long long NS = (long long)B * K * S;
  w.nblk = (int)cdiv((long long)B * S, SM_SUM_CHUNK);
  const long long hdr = 2ll * w.nblk * K * 4;
  const long long skel = sm_ws(nullptr, NS, iters).elems;
  w.part = (double*)scratch;
  w.coef = (float*)scratch + hdr;
  w.sp = w.coef + 32;
  w.skel_ws = w.sp + NS;
  w.keep = (uint8_t*)((float*)w.skel_ws + skel);
  w.elems = hdr + 32 + NS + skel + (NS + 3) / 4;
  return w;
}
static bool cld_shape_ok(int B, int H, int W, int D, int C, int K) {
  return B >= 1 && C >= 2 && C <= LTU_WIDE_MAXC && K >= 1 && K <= SM_MAX_K && sm_dims_ok((long long)B * K, H, W, D) &&
         sm_dims_ok((long long)B * C, H, W, D);
}

extern "C" long long ltu_loss_cldice_scratch_elems(int B, int H, int W, int D, int K, int iters) {
  if (!cld_shape_ok(B, H, W, D, 2, K) || iters < 1 || iters > SM_MAX_ITERS) return 0;
  return cld_ws(nullptr, B, (long long)H * W * D, K, iters).elems;
}

static SmSrc cld_src(const float* p, const int* classes, int K, long long S, int C) {
  SmSrc r;
  r.x = p; r.bstride = S * C; r.estride = C; r.K = K;
  for (int q = 0; q < SM_MAX_K; ++q) r.cls[q] = q < K ? classes[q] : 0;
  return r;
}

extern "C" int ltu_loss_cldice_fwd(const float* p, const uint8_t* label, const uint8_t* skel, const int* classes, const float* w, int K,
                                   int iters, void* scratch, long long scratch_elems, float* values, const float* base_total,
                                   const float* scale_dev, int B, int H, int W, int D, int C, ltu_stream_t s) {
  if (!cld_shape_ok(B, H, W, D, C, K)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || skel == nullptr || w == nullptr || scratch == nullptr || values == nullptr) return LTU_E_ARG;
  if (!sm_classes_ok(classes, K, C) || iters < 1 || iters > SM_MAX_ITERS) return LTU_E_ARG;
  CldCfg cfg;
  cfg.K = K;
  for (int k = 0; k < SM_MAX_K; ++k) {
    cfg.w[k] = k < K ? w[k] : 0.f;
    if (!isfinite(cfg.w[k])) return LTU_E_ARG;
  }
  const long long S = (long long)H * W * D;
  const CldWs cw = cld_ws(scratch, B, S, K, iters);
  if (scratch_elems < cw.elems) return LTU_E_ARG;
  if ((uintptr_t)scratch & 7) return LTU_E_ALIGN;      // the partials are doubles
  const SmDim g = sm_dim((long long)B * K, H, W, D);
  const SmSrc src = cld_src(p, classes, K, S, C);
  hipStream_t st = (hipStream_t)s;
  sm_skeleton_fwd(src, cw.sp, sm_ws(cw.skel_ws, g.NS, iters), g, iters, st);
  SmCls cc;
  cc.K = K;
  for (int q = 0; q < SM_MAX_K; ++q) cc.cls[q] = src.cls[q];
  hipLaunchKernelGGL(cld_sums_kernel, dim3(cw.nblk, K), dim3(256), 0, st, p, label, skel, (const float*)cw.sp, cc, cw.part, cw.keep, S,
                     (long long)B * S, C);
  hipLaunchKernelGGL(cld_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)cw.part, cw.nblk, cfg, values, cw.coef, base_total, scale_dev);
  return ltu_check_launch();
}

extern "C" int ltu_loss_cldice_bwd(const float* p, const uint8_t* label, const int* classes, int K, int iters, void* scratch,
                                   long long scratch_elems, const float* gscale, float* dp, int accumulate, int B, int H, int W, int D,
                                   int C, ltu_stream_t s) {
  if (!cld_shape_ok(B, H, W, D, C, K)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || scratch == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  if (!sm_classes_ok(classes, K, C) || iters < 1 || iters > SM_MAX_ITERS) return LTU_E_ARG;
  const long long S = (long long)H * W * D;
  const CldWs cw = cld_ws(scratch, B, S, K, iters);
  if (scratch_elems < cw.elems) return LTU_E_ARG;
  if ((uintptr_t)scratch & 7) return LTU_E_ALIGN;      // the partials are doubles
  const SmDim g = sm_dim((long long)B * K, H, W, D);
  const SmSrc src = cld_src(p, classes, K, S, C);
  hipStream_t st = (hipStream_t)s;
  if (!accumulate) {      // the channels the terms do not name receive no gradient: zeros, then the named channels are written
    hipError_t e = hipMemsetAsync(dp, 0, (size_t)B * S * C * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
  }
  SmSeed seed;
  seed.label = label; seed.coef = cw.coef; seed.gscale = gscale;
  SmOut o;
  o.out = dp; o.bstride = S * C; o.estride = C; o.K = K;
  for (int q = 0; q < SM_MAX_K; ++q) o.cls[q] = src.cls[q];
  o.skel = cw.keep; o.coef = cw.coef; o.gscale = gscale; o.accumulate = accumulate != 0;
  sm_skeleton_bwd(src, nullptr, seed, o, sm_ws(cw.skel_ws, g.NS, iters), g, iters, st);
  return ltu_check_launch();
}
