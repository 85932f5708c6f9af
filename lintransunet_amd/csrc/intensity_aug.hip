// The intensity half of nnU-Net's training augmentation on a batch of patches (no reference counterpart: the monai driver crops, flips
// and rot90s only): contrast about the patch mean, the gamma transform on the plain or the inverted image with the input's mean and
// standard deviation restored, and the low-resolution simulation.  Every statistic is one per (patch, channel) volume of `per`
// floats, stays on the device and is bit-reproducible: no floating-point atomics, a workgroup count that depends on `per` alone,
// fixed reduction trees, and a fold of the workgroups' records in index order.
//
//   ltu_patch_stats       {min, max, sum x, sum x^2} per volume (sums in fp64): one record per workgroup, then the fold
//   ltu_intensity_apply   per volume none / contrast / gamma / inverted gamma from the statistics of its input, and in the same pass
//                         the records of what it stored (for the rescale), then the fold
//   ltu_intensity_rescale y = (y - mean y) * std x / max(std y, 1e-7) + mean x in place, on the volumes that ask for it
//   ltu_lowres_gather     trilinear_up(nearest_exact_down(x)) as one 8-tap gather through per-axis index and weight tables
//
// ---- how a volume is split ---------------------------------------------------------------------------------------------------------
// Volume k begins at x + k * per, 16-byte aligned only when k * per is a multiple of 4.  It is cut into a scalar head of (-k per) & 3
// floats, nq whole 16-byte quads and a scalar tail of up to 3 floats.  Workgroup b of the volume's ia_blocks(per) takes the quads
// [b * qpb, (b + 1) * qpb), qpb = ceil(nq / blocks), 256 lanes striding through them; workgroup 0 also takes head and tail.  x and out
// share the split (both bases are 16-byte aligned), so a volume is loaded and stored in whole quads.
#include "common.h"

#define IA_THREADS 256
#define IA_CHUNK 4096            // floats per workgroup before the count is capped at LTU_PATCH_STATS_MAX_PARTS
static_assert(LTU_PATCH_STATS_MAX_PARTS == IA_THREADS, "the fold loads one record per lane");

static inline int ia_blocks(long long per) {
  const long long b = (per + IA_CHUNK - 1) / IA_CHUNK;
  return (int)(b < 1 ? 1 : b > LTU_PATCH_STATS_MAX_PARTS ? LTU_PATCH_STATS_MAX_PARTS : b);
}

struct IaAcc {
  float lo, hi;
  double s1, s2;
  __device__ __forceinline__ void init() { lo = INFINITY; hi = -INFINITY; s1 = 0.0; s2 = 0.0; }
  __device__ __forceinline__ void add(float v) {
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
    const double d = (double)v;
    s1 += d;
    s2 = fma(d, d, s2);
  }
};

// the workgroup's record {min, max, sum, sum of squares}: a fixed butterfly inside a wave, the 4 waves in order
__device__ __forceinline__ void ia_write(IaAcc a, double* __restrict__ rec) {
  __shared__ double red[4][IA_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) {
    a.lo = fminf(a.lo, __shfl_xor(a.lo, o));
    a.hi = fmaxf(a.hi, __shfl_xor(a.hi, o));
    a.s1 += __shfl_xor(a.s1, o);
    a.s2 += __shfl_xor(a.s2, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = (double)a.lo;
    red[1][wave] = (double)a.hi;
    red[2][wave] = a.s1;
    red[3][wave] = a.s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double lo = red[0][0], hi = red[1][0], s1 = red[2][0], s2 = red[3][0];
    for (int w = 1; w < IA_THREADS / 64; ++w) {
      lo = fmin(lo, red[0][w]);
      hi = fmax(hi, red[1][w]);
      s1 += red[2][w];
      s2 += red[3][w];
    }
    rec[0] = lo;
    rec[1] = hi;
    rec[2] = s1;
    rec[3] = s2;
  }
}

// F maps a loaded float to the stored one; STORE: write it to out; STATS: accumulate what was stored (or loaded)
template <bool STORE, bool STATS, class F>
__device__ __forceinline__ void ia_stream(const float* __restrict__ xk, float* __restrict__ ok, long long k, long long per, F f,
                                          double* __restrict__ rec) {
  long long head = (4 - ((k * per) & 3)) & 3;
  if (head > per) head = per;
  const long long nq = (per - head) >> 2, tail0 = head + 4 * nq;
  const long long qpb = (nq + gridDim.x - 1) / gridDim.x;
  const long long q0 = (long long)blockIdx.x * qpb, q1 = q0 + qpb < nq ? q0 + qpb : nq;
  IaAcc a;
  a.init();
  for (long long q = q0 + threadIdx.x; q < q1; q += IA_THREADS) {
    const float4 v = *reinterpret_cast<const float4*>(xk + head + 4 * q);
    const float4 y = make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
    if (STORE) *reinterpret_cast<float4*>(ok + head + 4 * q) = y;
    if (STATS) {
      a.add(y.x);
      a.add(y.y);
      a.add(y.z);
      a.add(y.w);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {           // lanes 0 .. 3 the head, 4 .. 7 the tail: at most 3 floats each
    const long long t = threadIdx.x & 3;
    const long long i = threadIdx.x < 4 ? t : tail0 + t;
    if (threadIdx.x < 4 ? t < head : i < per) {
      const float y = f(xk[i]);
      if (STORE) ok[i] = y;
      if (STATS) a.add(y);
    }
  }
  if (STATS) ia_write(a, rec);
}

__global__ void __launch_bounds__(IA_THREADS) patch_stats_kernel(const float* __restrict__ x, long long per, double* __restrict__ parts) {
  const long long k = blockIdx.y;
  ia_stream<false, true>(x + k * per, nullptr, k, per, [](float v) { return v; }, parts + (k * gridDim.x + blockIdx.x) * 4);
}

// one workgroup per volume: extrema by a tree (exact in any order), the two sums by one lane in index order
__global__ void __launch_bounds__(IA_THREADS) patch_fold_kernel(const double* __restrict__ parts, int nblk, double* __restrict__ stats) {
  __shared__ double sm[2][LTU_PATCH_STATS_MAX_PARTS];
  __shared__ double ext[2][IA_THREADS / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  double lo = INFINITY, hi = -INFINITY;
  if (tid < nblk) {
    const double* r = parts + ((long long)k * nblk + tid) * 4;
    lo = r[0];
    hi = r[1];
    sm[0][tid] = r[2];
    sm[1][tid] = r[3];
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o));
    hi = fmax(hi, __shfl_xor(hi, o));
  }
  if ((tid & 63) == 0) {
    ext[0][tid >> 6] = lo;
    ext[1][tid >> 6] = hi;
  }
  __syncthreads();
  if (tid == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < nblk; ++i) {
      s1 += sm[0][i];
      s2 += sm[1][i];
    }
    for (int w = 1; w < IA_THREADS / 64; ++w) {
      lo = fmin(lo, ext[0][w]);
      hi = fmax(hi, ext[1][w]);
    }
    double* o = stats + 4 * (long long)k;
    o[0] = lo;
    o[1] = hi;
    o[2] = s1;
    o[3] = s2;
  }
}

// ---- ltu_intensity_apply -------------------------------------------------------------------------------------------------------------
// The op is uniform in a workgroup.  contrast: clip((x - m) f + m, lo, hi) with m = (float)(sum / per).  gamma on u = x or -x:
// ((u - lo_u) / max(r, 1e-7))^g r + lo_u, the power as exp2(g log2 t) on the hardware transcendentals (t = 0: log2 = -inf, exp2 = 0);
// a volume without a range (max == min) is copied.  op none returns the loaded float: the same bits.
struct IaArgs {
  int op[LTU_INTENSITY_AUG_MAX_N];
  float par[LTU_INTENSITY_AUG_MAX_N];
};

template <bool STATS>
__global__ void __launch_bounds__(IA_THREADS) intensity_apply_kernel(const float* __restrict__ x, float* __restrict__ out, IaArgs c,
                                                                     const double* __restrict__ stats, long long per,
                                                                     double* __restrict__ parts) {
  const long long k = blockIdx.y;
  const double* st = stats + 4 * k;
  const float lo = (float)st[0], hi = (float)st[1], m = (float)(st[2] / (double)per);       // the extrema were floats: exact
  const float p = c.par[k];
  int op = c.op[k];
  if (op >= LTU_IAUG_GAMMA && !(hi > lo)) op = LTU_IAUG_NONE;
  const bool inv = op == LTU_IAUG_GAMMA_INV;
  const float r = hi - lo, den = fmaxf(r, 1e-7f), ulo = inv ? -hi : lo;
  const float* xk = x + k * per;
  float* ok = out + k * per;
  double* rec = STATS ? parts + (k * gridDim.x + blockIdx.x) * 4 : nullptr;
  if (op == LTU_IAUG_CONTRAST)
    ia_stream<true, STATS>(xk, ok, k, per, [=](float v) { return fminf(fmaxf(fmaf(v - m, p, m), lo), hi); }, rec);
  else if (op >= LTU_IAUG_GAMMA)
    ia_stream<true, STATS>(xk, ok, k, per, [=](float v) {
      const float t = ((inv ? -v : v) - ulo) / den;
      const float w = fmaf(__builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(t)), r, ulo);
      return inv ? -w : w;
    }, rec);
  else
    ia_stream<true, STATS>(xk, ok, k, per, [](float v) { return v; }, rec);
}

struct IaOn {
  unsigned char on[LTU_INTENSITY_AUG_MAX_N];
};

// y <- (y - mean y) a + mean x, a = std x / max(std y, 1e-7) from the two records in fp64 (population moments: the estimator cancels)
__global__ void __launch_bounds__(IA_THREADS) intensity_rescale_kernel(float* __restrict__ y, IaOn c, const double* __restrict__ sx,
                                                                       const double* __restrict__ sy, long long per) {
  const long long k = blockIdx.y;
  const double* a = sx + 4 * k;
  const double* b = sy + 4 * k;
  if (!c.on[k] || !(a[1] > a[0])) return;             // not asked for, or a constant volume: left as it is
  const double n = (double)per, mx = a[2] / n, my = b[2] / n;
  const double vx = fmax(a[3] / n - mx * mx, 0.0), vy = fmax(b[3] / n - my * my, 0.0);
  const float g = (float)(sqrt(vx) / fmax(sqrt(vy), 1e-7)), fmx = (float)mx, fmy = (float)my;
  float* yk = y + k * per;
  ia_stream<true, false>(yk, yk, k, per, [=](float v) { return fmaf(v - fmy, g, fmx); }, nullptr);
}

// ---- ltu_lowres_gather -----------------------------------------------------------------------------------------------------------------
// A workgroup takes LR_CHUNK consecutive voxels of one (volume, x) plane [W][D], a lane every 256th of them: the 64 lanes of a wave
// store 64 consecutive floats and read, per tap, the few cache lines under them (a lane that owned 4 consecutive voxels would
// spread every tap load of the wave over 4 times as many lines).  The workgroup stages the volume's W and D tables and its own x
// entry in LDS, one 16-byte record per output index: {offset of the lower tap, offset of the upper tap, weight of the upper tap},
// the indices clamped into the axis (any table content gives addresses inside the volume) and multiplied by the axis's stride.  A
// voxel is then
//   w000 v000 + w001 v001 + ... + w111 v111,  w = (wx wy) wz with (1 - l | l) per axis, taps in the order x, y, z (z fastest):
// the first product rounded, every further tap one fused multiply-add, and a tap of weight 0 is left out.  With l = 0 on all three
// axes that is 1 * v000: the input's bits.  (y, z) advance by 256 voxels with one carry; a lane past the plane's end computes on
// the last row and stores nothing, so the loop body has no branch around its loads.
#define LR_CHUNK 4096

__global__ void __launch_bounds__(IA_THREADS) lowres_gather_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                   const int* __restrict__ tab, int H, int W, int D) {
  extern __shared__ int4 lr_lds[];                     // [1 + W + D]: entry 0 the x row's, then the W table, then the D table
  const int k = blockIdx.z, xo = blockIdx.y;
  const int L = H + W + D, LL = 1 + W + D, plane = W * D;
  const int* tk = tab + (long long)k * 3 * L;
  for (int e = threadIdx.x; e < LL; e += IA_THREADS) {
    const int src = e == 0 ? xo : H + e - 1;
    const int S = e == 0 ? H : e <= W ? W : D;
    const int stride = e == 0 ? plane : e <= W ? D : 1;
    lr_lds[e] = make_int4(min(max(tk[src], 0), S - 1) * stride, min(max(tk[L + src], 0), S - 1) * stride, tk[2 * L + src], 0);
  }
  __syncthreads();
  const float* xk = x + (long long)k * H * plane;
  float* ok = out + ((long long)k * H + xo) * plane;
  const int4 ex = lr_lds[0];
  const float lx = __int_as_float(ex.z);
  const float* px[2] = {xk + ex.x, xk + ex.y};
  int p = blockIdx.x * LR_CHUNK + threadIdx.x;
  int y = p / D, z = p - y * D;
  const int dy = IA_THREADS / D, dz = IA_THREADS - dy * D;
#pragma unroll 4
  for (int it = 0; it < LR_CHUNK / IA_THREADS; ++it) {
    const int4 ey = lr_lds[1 + min(y, W - 1)], ez = lr_lds[1 + W + z];
    const float ly = __int_as_float(ey.z), lz = __int_as_float(ez.z);
    const float wxy[4] = {(1.f - lx) * (1.f - ly), (1.f - lx) * ly, lx * (1.f - ly), lx * ly};
    const int oy[2] = {ey.x, ey.y}, oz[2] = {ez.x, ez.y};
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float w = wxy[t >> 1] * ((t & 1) ? lz : 1.f - lz);
      const float v = px[t >> 2][oy[(t >> 1) & 1] + oz[t & 1]];
      if (t == 0) acc = w * v;
      else acc = w != 0.f ? fmaf(w, v, acc) : acc;
    }
    if (p < plane) ok[p] = acc;
    p += IA_THREADS;
    y += dy;
    z += dz;
    if (z >= D) {
      z -= D;
      ++y;
    }
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------------
static bool ia_per_ok(long long per) { return per >= 1 && per < (1LL << 31); }

extern "C" long long ltu_patch_stats_parts_elems(int n, long long per) {
  if (n < 1 || n > 65535 || !ia_per_ok(per)) return 0;
  return 4LL * n * ia_blocks(per);
}

extern "C" int ltu_patch_stats(const float* x, int n, long long per, double* parts, long long parts_elems, double* stats,
                               ltu_stream_t s) {
  if (x == nullptr || parts == nullptr || stats == nullptr || n < 0) return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (n > 65535 || !ia_per_ok(per)) return LTU_E_SHAPE;
  const int nblk = ia_blocks(per);
  if (parts_elems < 4LL * n * nblk) return LTU_E_ARG;
  if (((uintptr_t)x & 15) != 0 || ((uintptr_t)parts & 7) != 0 || ((uintptr_t)stats & 7) != 0) return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(patch_stats_kernel, dim3(nblk, n), dim3(IA_THREADS), 0, st, x, per, parts);
  hipLaunchKernelGGL(patch_fold_kernel, dim3(n), dim3(IA_THREADS), 0, st, parts, nblk, stats);
  return ltu_check_launch();
}

extern "C" int ltu_intensity_apply(const float* x, float* out, const int* ops, const float* params, const double* stats, int n,
                                   long long per, double* parts, long long parts_elems, double* out_stats, ltu_stream_t s) {
  if (x == nullptr || out == nullptr || ops == nullptr || params == nullptr || stats == nullptr || n < 0 ||
      n > LTU_INTENSITY_AUG_MAX_N || (out_stats != nullptr && parts == nullptr))
    return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (!ia_per_ok(per)) return LTU_E_SHAPE;
  const int nblk = ia_blocks(per);
  if (out_stats != nullptr && parts_elems < 4LL * n * nblk) return LTU_E_ARG;
  IaArgs c;
  for (int k = 0; k < n; ++k) {
    if (ops[k] < LTU_IAUG_NONE || ops[k] > LTU_IAUG_GAMMA_INV || !(params[k] - params[k] == 0.f)) return LTU_E_ARG;
    c.op[k] = params[k] > 0.f ? ops[k] : LTU_IAUG_NONE;          // a non-positive parameter leaves the volume as it is
    c.par[k] = params[k];
  }
  if (((uintptr_t)x & 15) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)stats & 7) != 0 ||
      (out_stats != nullptr && (((uintptr_t)parts & 7) != 0 || ((uintptr_t)out_stats & 7) != 0)))
    return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  if (out_stats != nullptr) {
    hipLaunchKernelGGL(intensity_apply_kernel<true>, dim3(nblk, n), dim3(IA_THREADS), 0, st, x, out, c, stats, per, parts);
    hipLaunchKernelGGL(patch_fold_kernel, dim3(n), dim3(IA_THREADS), 0, st, parts, nblk, out_stats);
  } else {
    hipLaunchKernelGGL(intensity_apply_kernel<false>, dim3(nblk, n), dim3(IA_THREADS), 0, st, x, out, c, stats, per, nullptr);
  }
  return ltu_check_launch();
}

extern "C" int ltu_intensity_rescale(float* y, const unsigned char* on, const double* stats_x, const double* stats_y, int n,
                                     long long per, ltu_stream_t s) {
  if (y == nullptr || on == nullptr || stats_x == nullptr || stats_y == nullptr || n < 0 || n > LTU_INTENSITY_AUG_MAX_N)
    return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (!ia_per_ok(per)) return LTU_E_SHAPE;
  if (((uintptr_t)y & 15) != 0 || ((uintptr_t)stats_x & 7) != 0 || ((uintptr_t)stats_y & 7) != 0) return LTU_E_ALIGN;
  IaOn c;
  bool any = false;
  for (int k = 0; k < n; ++k) {
    c.on[k] = on[k] != 0;
    any = any || c.on[k];
  }
  if (!any) return LTU_OK;
  hipLaunchKernelGGL(intensity_rescale_kernel, dim3(ia_blocks(per), n), dim3(IA_THREADS), 0, (hipStream_t)s, y, c, stats_x, stats_y, per);
  return ltu_check_launch();
}

extern "C" int ltu_lowres_gather(const float* x, float* out, const int* tables, int n, int H, int W, int D, ltu_stream_t s) {
  if (x == nullptr || out == nullptr || x == out || tables == nullptr || n < 0) return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (H < 1 || W < 1 || D < 1 || H > LTU_LOWRES_MAX_EXTENT || W > LTU_LOWRES_MAX_EXTENT || D > LTU_LOWRES_MAX_EXTENT || n > 65535 ||
      (long long)n * H * W * D >= (1LL << 40))
    return LTU_E_SHAPE;
  if (((uintptr_t)x & 3) != 0 || ((uintptr_t)tables & 3) != 0 || ((uintptr_t)out & 3) != 0) return LTU_E_ALIGN;
  const dim3 grid(cdiv((long long)W * D, LR_CHUNK), H, n);
  const int smem = (1 + W + D) * (int)sizeof(int4);          // at most 32.8 KB
  hipLaunchKernelGGL(lowres_gather_kernel, grid, dim3(IA_THREADS), smem, (hipStream_t)s, x, out, tables, H, W, D);
  return ltu_check_launch();
}
