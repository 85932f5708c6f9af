// Top-k cross-entropy of one decoder level (nnU-Net's TopKLoss, "hard-voxel mining"): the mean of the per-voxel cross-entropy
//     l = -log(max(p[label], 1e-6))            (0 and no gradient where label >= C)
// over the k = min(max(floor(frac N), 1), N) hardest of the N = B S voxels of the batch.  With tau the k-th largest l, n_gt = #{l > tau}
// and n_eq = #{l == tau}:   value = (sum_{l > tau} l + (k - n_gt) tau) / k,   total = base + scale w value,
// and a voxel weighs 1 / k above tau, 0 below it and (k - n_gt) / (n_eq k) on it: the symmetric subgradient.  torch.topk picks
// among tied voxels arbitrarily; sharing the remaining weight among all of them is what makes the result a function of the input.
//
// tau comes from an exact radix select on the bit pattern of l (l >= 0: unsigned order is float order): three histogram passes
// over the digits [30:20], [19:9], [8:0] of the key, each narrowing to the one bin that holds rank k.  Counts are integers (LDS
// and global integer atomics: sums of integers do not depend on their order), so tau, n_gt and n_eq are exact and two calls agree
// bit for bit.  No floating-point atomics: sum_{l > tau} l is made of per-workgroup partials folded in a fixed order (the keys
// above the selected bin of pass j are known to be above tau, and are summed by pass j + 1) plus, for the last digit, count x
// value straight from the histogram.
//
// Bytes: pass 1 reads p and label once and leaves the keys in scratch (4 C + 1 + 4 bytes a voxel), passes 2 and 3 read the keys
// (4 + 4): 25 bytes a voxel at C = 3 against 39 for three passes over p.  The backward reads keys and labels and touches p and dp
// only at the selected voxels, one channel each.
//
// The hot bin: late in training most voxels have p == 1.0 exactly, l = 0, and one bin takes most of the batch (voxels with
// label >= C land there too).  Bin 0 is therefore counted with a wave ballot into a register, no atomic at all; of the other
// keys of a wave instruction those equal to the first one go in as one add (the clamp value -log 1e-6 is the other value that
// ties in bulk); the rest are one LDS add a lane.  A workgroup flushes one global add per non-empty bin.  From pass 2 on only
// keys inside the selected bin are counted.
#include "common.h"

#include <math.h>

#define TK_THREADS 256
#define TK_MAX_BLOCKS 1024        // workgroups of every pass (grid-stride): at most this many adds meet on one global bin
#define TK_BINS1 2048             // key bits [30:20] (bit 31 is clear: l >= 0, -0.0 canonicalised)
#define TK_BINS2 2048             // key bits [19:9]
#define TK_BINS3 512              // key bits [8:0]
// scratch, in 4-byte elements
#define TK_HIST1 0
#define TK_HIST2 (TK_HIST1 + TK_BINS1)
#define TK_HIST3 (TK_HIST2 + TK_BINS2)
#define TK_NHIST (TK_HIST3 + TK_BINS3)
#define TK_REC 6144               // selection record, 16 words (TkRec)
#define TK_PART (TK_REC + 16)     // doubles: [2][TK_MAX_BLOCKS] partial sums of passes 2 and 3
#define TK_KEYS (TK_PART + 4 * TK_MAX_BLOCKS)      // N keys, on a 16-byte boundary

enum TkRec { TK_D1 = 0, TK_K1 = 1, TK_GT1 = 2, TK_D2 = 3, TK_K2 = 4, TK_GT2 = 5, TK_TAU = 8, TK_K = 9, TK_NGT = 10, TK_NEQ = 11 };

// k of the definition; a device value out of range is clamped, a non-finite one gives N
__device__ __forceinline__ uint32_t tk_count(float frac, const float* __restrict__ frac_dev, long long N) {
  const double f = (double)(frac_dev ? frac_dev[0] : frac);
  if (!isfinite(f)) return (uint32_t)N;
  const double kk = floor(f * (double)N);
  return kk < 1.0 ? 1u : kk > (double)N ? (uint32_t)N : (uint32_t)kk;
}

// One wave instruction's keys into the workgroup's LDS histogram.  Called by all 64 lanes together (`valid` masks a lane out).
// zc: the wave's count of bin 0, the same in every lane.
__device__ __forceinline__ void tk_hist_add(uint32_t* __restrict__ h, uint32_t bin, bool valid, uint32_t& zc) {
  zc += (uint32_t)__popcll(__ballot(valid && bin == 0u));
  const bool rest = valid && bin != 0u;
  const unsigned long long mr = __ballot(rest);
  if (mr == 0ull) return;                                     // wave-uniform
  const int src = __ffsll((long long)mr) - 1;
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, src);
  const bool same = rest && bin == b0;
  const unsigned long long ms = __ballot(same);
  if ((int)(threadIdx.x & 63) == src) atomicAdd(&h[b0], (uint32_t)__popcll(ms));
  else if (rest && !same) atomicAdd(&h[bin], 1u);
}

// zc of every wave into bin 0, then one global add per non-empty bin
__device__ __forceinline__ void tk_hist_flush(uint32_t* __restrict__ h, uint32_t zc, uint32_t* __restrict__ ghist, int nbins) {
  if ((threadIdx.x & 63) == 0 && zc) atomicAdd(&h[0], zc);
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += TK_THREADS) {
    const uint32_t v = h[b];
    if (v) atomicAdd(&ghist[b], v);
  }
}

// The bin of `hist` (NB bins) that holds rank k counted from the top (1 <= k <= sum of hist) and gt = the count of the bins above
// it.  All TK_THREADS threads; thread t owns the PER bins below NB - t PER.  sh: TK_THREADS + 2 words of LDS.
template <int NB>
__device__ __forceinline__ void tk_select(const uint32_t* __restrict__ hist, uint32_t k, uint32_t* __restrict__ sh, uint32_t& d, uint32_t& gt) {
  constexpr int PER = NB / TK_THREADS;
  const int t = threadIdx.x;
  uint32_t hv[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    hv[j] = hist[NB - 1 - (t * PER + j)];                   // j-th bin from the top of this thread's range
    s += hv[j];
  }
  sh[t] = s;
  __syncthreads();
  for (int off = 1; off < TK_THREADS; off <<= 1) {
    const uint32_t v = t >= off ? sh[t - off] : 0u;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  uint32_t c = incl - s;                                      // count of all bins above this thread's
  if (c < k && k <= incl) {                                   // exactly one thread
    bool found = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!found && c + hv[j] >= k) {
        sh[TK_THREADS] = (uint32_t)(NB - 1 - (t * PER + j));
        sh[TK_THREADS + 1] = c;
        found = true;
      }
      if (!found) c += hv[j];
    }
  }
  __syncthreads();
  d = sh[TK_THREADS];
  gt = sh[TK_THREADS + 1];
  __syncthreads();
}

// sum of a workgroup's per-thread values in a fixed order; the result in thread 0
__device__ __forceinline__ double tk_block_sum(double v, double* __restrict__ red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = TK_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(TK_THREADS) tk_zero_kernel(uint32_t* __restrict__ scr) {
  const int i = blockIdx.x * TK_THREADS + threadIdx.x;
  if (i < TK_NHIST) scr[i] = 0u;
}

// the key of a voxel: the bits of l, -0.0 (p == 1.0) and anything below it (p > 1) as +0.0
__device__ __forceinline__ uint32_t tk_key(float pl, bool labelled) {
  const float l = labelled ? 0.f - logf(fmaxf(pl, 1e-6f)) : 0.f;
  const uint32_t key = __float_as_uint(l);
  return (key & 0x80000000u) ? 0u : key;
}

// pass 1: p f32 [N][C], label u8 [N] -> keys [N] and the histogram of key bits [30:20].  V4: four voxels a thread and trip (N % 4
// == 0, 16-byte aligned p and keys, 4-byte aligned label): one 4-byte label load, C 16-byte loads, one 16-byte store
template <int C, bool V4>
__global__ void __launch_bounds__(TK_THREADS) tk_pass1_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label,
                                                              uint32_t* __restrict__ scr, long long N) {
  __shared__ uint32_t h[TK_BINS1];
  for (int b = threadIdx.x; b < TK_BINS1; b += TK_THREADS) h[b] = 0u;
  __syncthreads();
  uint32_t* __restrict__ keys = scr + TK_KEYS;
  uint32_t zc = 0;
  constexpr int V = V4 ? 4 : 1;
  for (long long base = (long long)blockIdx.x * TK_THREADS * V; base < N; base += (long long)gridDim.x * TK_THREADS * V) {
    const long long i = base + (long long)threadIdx.x * V;
    const bool valid = i < N;
    if constexpr (V4) {
      uint32_t k4[4] = {0u, 0u, 0u, 0u};
      if (valid) {
        const uint32_t labs = *reinterpret_cast<const uint32_t*>(label + i);
        float f[4 * C];
#pragma unroll
        for (int q = 0; q < C; ++q) {
          const float4 t = *reinterpret_cast<const float4*>(p + i * C + 4 * q);
          f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int lab = (int)((labs >> (8 * j)) & 255u);
          float pl = 1.f;
#pragma unroll
          for (int c = 0; c < C; ++c) pl = lab == c ? f[j * C + c] : pl;
          k4[j] = tk_key(pl, lab < C);
        }
        *reinterpret_cast<uint4*>(keys + i) = make_uint4(k4[0], k4[1], k4[2], k4[3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tk_hist_add(h, k4[j] >> 20, valid, zc);
    } else {
      uint32_t key = 0u;
      if (valid) {
        const int lab = label[i];
        const float pl = lab < C ? p[i * C + lab] : 1.f;
        key = tk_key(pl, lab < C);
        keys[i] = key;
      }
      tk_hist_add(h, key >> 20, valid, zc);
    }
  }
  tk_hist_flush(h, zc, scr + TK_HIST1, TK_BINS1);
}

// passes 2 and 3 over the keys.  Every workgroup first repeats the selection of the pass before it (a scan of one histogram), then
// counts the next digit of the keys inside the selected bin and sums the keys that this selection has put above tau.
template <int LEVEL, bool V4>
__global__ void __launch_bounds__(TK_THREADS) tk_pass_kernel(uint32_t* __restrict__ scr, long long N, float frac,
                                                             const float* __restrict__ frac_dev) {
  __shared__ uint32_t h[LEVEL == 2 ? TK_BINS2 : TK_BINS3];
  __shared__ uint32_t sh[TK_THREADS + 2];
  __shared__ double red[TK_THREADS];
  constexpr int NB = LEVEL == 2 ? TK_BINS2 : TK_BINS3;
  for (int b = threadIdx.x; b < NB; b += TK_THREADS) h[b] = 0u;
  uint32_t* __restrict__ rec = scr + TK_REC;
  uint32_t d1, d2 = 0u, gt;
  if constexpr (LEVEL == 2) {
    const uint32_t k = tk_count(frac, frac_dev, N);
    tk_select<TK_BINS1>(scr + TK_HIST1, k, sh, d1, gt);
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec[TK_D1] = d1; rec[TK_K1] = k - gt; rec[TK_GT1] = gt; rec[TK_K] = k; }
  } else {
    d1 = rec[TK_D1];
    const uint32_t k1 = rec[TK_K1];
    tk_select<TK_BINS2>(scr + TK_HIST2, k1, sh, d2, gt);
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec[TK_D2] = d2; rec[TK_K2] = k1 - gt; rec[TK_GT2] = rec[TK_GT1] + gt; }
  }
  // (tk_select ends on a barrier: h is zeroed)
  const uint32_t pre = LEVEL == 2 ? d1 : (d1 << 11) | d2;    // the selected key prefix, of 11 or 22 bits
  const uint32_t* __restrict__ keys = scr + TK_KEYS;
  uint32_t zc = 0;
  float acc = 0.f;
  auto one = [&](uint32_t key, bool valid) {
    if constexpr (LEVEL == 2) {
      const uint32_t top = key >> 20;
      if (valid && top > pre) acc += __uint_as_float(key);
      tk_hist_add(h, (key >> 9) & 2047u, valid && top == pre, zc);
    } else {
      const uint32_t top = key >> 9;
      if (valid && (key >> 20) == d1 && top > pre) acc += __uint_as_float(key);
      tk_hist_add(h, key & 511u, valid && top == pre, zc);
    }
  };
  constexpr int V = V4 ? 4 : 1;
  for (long long base = (long long)blockIdx.x * TK_THREADS * V; base < N; base += (long long)gridDim.x * TK_THREADS * V) {
    const long long i = base + (long long)threadIdx.x * V;
    const bool valid = i < N;
    if constexpr (V4) {
      const uint4 k4 = valid ? *reinterpret_cast<const uint4*>(keys + i) : make_uint4(0u, 0u, 0u, 0u);
      one(k4.x, valid); one(k4.y, valid); one(k4.z, valid); one(k4.w, valid);
    } else {
      one(valid ? keys[i] : 0u, valid);
    }
  }
  tk_hist_flush(h, zc, scr + (LEVEL == 2 ? TK_HIST2 : TK_HIST3), NB);
  const double v = tk_block_sum((double)acc, red);
  if (threadIdx.x == 0) reinterpret_cast<double*>(scr + TK_PART)[(LEVEL - 2) * TK_MAX_BLOCKS + blockIdx.x] = v;
}

// one workgroup: the last selection, the fold of the partials in workgroup order, the values and the record of the backward
__global__ void __launch_bounds__(TK_THREADS) tk_finalize_kernel(uint32_t* __restrict__ scr, int nblk, long long N, float* __restrict__ values,
                                                                 const float* __restrict__ base_total, float w,
                                                                 const float* __restrict__ scale_dev) {
  __shared__ uint32_t sh[TK_THREADS + 2];
  __shared__ double red[TK_THREADS];
  uint32_t* __restrict__ rec = scr + TK_REC;
  const uint32_t* __restrict__ hist3 = scr + TK_HIST3;
  const uint32_t d1 = rec[TK_D1], d2 = rec[TK_D2], k2 = rec[TK_K2], k = rec[TK_K];
  uint32_t d3, gt;
  tk_select<TK_BINS3>(hist3, k2, sh, d3, gt);
  const uint32_t prefix = (d1 << 20) | (d2 << 9);
  const double* __restrict__ part = reinterpret_cast<const double*>(scr + TK_PART);
  double acc = 0.0;
  for (int g = threadIdx.x; g < nblk; g += TK_THREADS) acc += part[g];
  for (int g = threadIdx.x; g < nblk; g += TK_THREADS) acc += part[TK_MAX_BLOCKS + g];
  for (uint32_t b = threadIdx.x; b < TK_BINS3; b += TK_THREADS)
    if (b > d3) acc += (double)hist3[b] * (double)__uint_as_float(prefix | b);      // a bin of the last digit is one value
  const double above = tk_block_sum(acc, red);
  if (threadIdx.x != 0) return;
  const uint32_t n_gt = rec[TK_GT2] + gt, n_eq = hist3[d3];
  const float tau = __uint_as_float(prefix | d3);
  const float value = (float)((above + (double)(k - n_gt) * (double)tau) / (double)k);
  rec[TK_TAU] = prefix | d3; rec[TK_NGT] = n_gt; rec[TK_NEQ] = n_eq;
  values[1] = value;
  values[2] = tau;
  const float sw = (scale_dev ? scale_dev[0] : 1.f) * w;
  values[0] = (base_total ? base_total[0] : 0.f) + sw * value;
}

// dp[i][label] gets g scale w weight (-1 / p) where p >= 1e-6.  ACC: added, and voxels below tau are not touched at all; else
// every channel is written.  V4 (ACC only): four keys and labels a load.
template <int C, bool ACC, bool V4>
__global__ void __launch_bounds__(TK_THREADS) tk_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label,
                                                            const uint32_t* __restrict__ scr, float w, const float* __restrict__ scale_dev,
                                                            const float* __restrict__ gscale, float* __restrict__ dp, long long N) {
  const uint32_t* __restrict__ rec = scr + TK_REC;
  const uint32_t* __restrict__ keys = scr + TK_KEYS;
  const uint32_t tau = rec[TK_TAU], k = rec[TK_K], n_gt = rec[TK_NGT], n_eq = rec[TK_NEQ];
  const float gs = gscale[0] * ((scale_dev ? scale_dev[0] : 1.f) * w);
  const float cgt = gs * (float)(1.0 / (double)k);
  const float ceq = gs * (float)((double)(k - n_gt) / ((double)n_eq * (double)k));
  auto term = [&](long long i, uint32_t key, int lab) -> float {      // the voxel's gradient in channel lab (lab < C)
    const float coef = key > tau ? cgt : ceq;
    const float pl = p[i * C + lab];
    return pl >= 1e-6f ? coef * (-1.f / pl) : 0.f;
  };
  if constexpr (V4) {
    for (long long i = ((long long)blockIdx.x * TK_THREADS + threadIdx.x) * 4; i < N; i += (long long)gridDim.x * TK_THREADS * 4) {
      const uint4 k4 = *reinterpret_cast<const uint4*>(keys + i);
      const uint32_t kk[4] = {k4.x, k4.y, k4.z, k4.w};
      if (kk[0] < tau && kk[1] < tau && kk[2] < tau && kk[3] < tau) continue;
      const uint32_t labs = *reinterpret_cast<const uint32_t*>(label + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lab = (int)((labs >> (8 * j)) & 255u);
        if (kk[j] >= tau && lab < C) dp[(i + j) * C + lab] += term(i + j, kk[j], lab);
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * TK_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * TK_THREADS) {
      const uint32_t key = keys[i];
      const int lab = label[i];
      const bool sel = key >= tau && lab < C;
      if constexpr (ACC) {
        if (sel) dp[i * C + lab] += term(i, key, lab);
      } else {
        const float v = sel ? term(i, key, lab) : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dp[i * C + c] = c == lab ? v : 0.f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
static int tk_shape(int B, long long S, int C, long long* N) {
  if (C < 2 || C > LTU_WIDE_MAXC || B < 1 || S < 1) return LTU_E_SHAPE;
  if (S > 2147483647LL || (long long)B * S > 2147483647LL) return LTU_E_SHAPE;
  *N = (long long)B * S;
  return LTU_OK;
}
static unsigned tk_blocks(long long N, int per_thread, long long cap = TK_MAX_BLOCKS) {
  const long long g = (N + (long long)TK_THREADS * per_thread - 1) / ((long long)TK_THREADS * per_thread);
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

extern "C" long long ltu_loss_topk_scratch_elems(int B, long long S) {
  long long N;
  if (tk_shape(B, S, 2, &N) != LTU_OK) return 0;
  return TK_KEYS + (N + 3) / 4 * 4;
}

extern "C" int ltu_loss_topk_fwd(const float* p, const uint8_t* label, void* scratch, long long scratch_elems, float* values,
                                 const float* base_total, float w, float frac, const float* frac_dev, const float* scale_dev, int B,
                                 long long S, int C, ltu_stream_t s) {
  long long N;
  const int rc = tk_shape(B, S, C, &N);
  if (rc != LTU_OK) return rc;
  if (p == nullptr || label == nullptr || scratch == nullptr || values == nullptr) return LTU_E_ARG;
  if (scratch_elems < ltu_loss_topk_scratch_elems(B, S) || !isfinite(w)) return LTU_E_ARG;
  if (frac_dev == nullptr && !(frac > 0.f && frac <= 1.f)) return LTU_E_ARG;
  if ((uintptr_t)scratch & 15) return LTU_E_ALIGN;
  uint32_t* scr = (uint32_t*)scratch;
  hipStream_t st = (hipStream_t)s;
  const bool kv4 = N % 4 == 0;                                                        // the keys sit on a 16-byte boundary
  const bool pv4 = kv4 && !((uintptr_t)p & 15) && !((uintptr_t)label & 3);
  const unsigned g1 = tk_blocks(N, pv4 ? 4 : 1), g2 = tk_blocks(N, kv4 ? 4 : 1);
  hipLaunchKernelGGL(tk_zero_kernel, dim3((TK_NHIST + TK_THREADS - 1) / TK_THREADS), dim3(TK_THREADS), 0, st, scr);
  LTU_DISPATCH_C(C, {
    if (pv4)
      hipLaunchKernelGGL((tk_pass1_kernel<(CT < 2 ? 2 : CT), true>), dim3(g1), dim3(TK_THREADS), 0, st, p, label, scr, N);
    else
      hipLaunchKernelGGL((tk_pass1_kernel<(CT < 2 ? 2 : CT), false>), dim3(g1), dim3(TK_THREADS), 0, st, p, label, scr, N);
  });
  if (kv4) {
    hipLaunchKernelGGL((tk_pass_kernel<2, true>), dim3(g2), dim3(TK_THREADS), 0, st, scr, N, frac, frac_dev);
    hipLaunchKernelGGL((tk_pass_kernel<3, true>), dim3(g2), dim3(TK_THREADS), 0, st, scr, N, frac, frac_dev);
  } else {
    hipLaunchKernelGGL((tk_pass_kernel<2, false>), dim3(g2), dim3(TK_THREADS), 0, st, scr, N, frac, frac_dev);
    hipLaunchKernelGGL((tk_pass_kernel<3, false>), dim3(g2), dim3(TK_THREADS), 0, st, scr, N, frac, frac_dev);
  }
  hipLaunchKernelGGL(tk_finalize_kernel, dim3(1), dim3(TK_THREADS), 0, st, scr, (int)g2, N, values, base_total, w, scale_dev);
  return ltu_check_launch();
}

extern "C" int ltu_loss_topk_bwd(const float* p, const uint8_t* label, const void* scratch, long long scratch_elems, float w,
                                 const float* scale_dev, const float* gscale, float* dp, int accumulate, int B, long long S, int C,
                                 ltu_stream_t s) {
  long long N;
  const int rc = tk_shape(B, S, C, &N);
  if (rc != LTU_OK) return rc;
  if (p == nullptr || label == nullptr || scratch == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  if (scratch_elems < ltu_loss_topk_scratch_elems(B, S) || !isfinite(w)) return LTU_E_ARG;
  if ((uintptr_t)scratch & 15) return LTU_E_ALIGN;
  const uint32_t* scr = (const uint32_t*)scratch;
  hipStream_t st = (hipStream_t)s;
  const bool v4 = accumulate && N % 4 == 0 && !((uintptr_t)label & 3);
  const unsigned g = tk_blocks(N, v4 ? 4 : 1, 2048);        // nothing meets on an address here
  LTU_DISPATCH_C(C, {
    if (v4)
      hipLaunchKernelGGL((tk_bwd_kernel<(CT < 2 ? 2 : CT), true, true>), dim3(g), dim3(TK_THREADS), 0, st, p, label, scr, w, scale_dev, gscale, dp, N);
    else if (accumulate)
      hipLaunchKernelGGL((tk_bwd_kernel<(CT < 2 ? 2 : CT), true, false>), dim3(g), dim3(TK_THREADS), 0, st, p, label, scr, w, scale_dev, gscale, dp, N);
    else
      hipLaunchKernelGGL((tk_bwd_kernel<(CT < 2 ? 2 : CT), false, false>), dim3(g), dim3(TK_THREADS), 0, st, p, label, scr, w, scale_dev, gscale, dp, N);
  });
  return ltu_check_launch();
}
