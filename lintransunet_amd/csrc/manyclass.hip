// Training path for 5 .. 8 classes on gfx950: mask-head softmax, final head (window un-embedding + softmax) and the
// deep-supervision loss of one level, forward and backward.  The class count is a template argument everywhere: per-thread
// arrays are indexed by unrolled loops only (a run-time class loop over them would put them in scratch memory or serialise
// the loads, see the CT = 0 path of pointwise.hip), and all loads of a row / coarse voxel are issued before the arithmetic.
//
// C <= 4 keeps the kernels of pointwise.hip and loss.hip; ltu_head_softmax_* and ltu_final_softmax_* hand C = 5 .. 8 over to the
// launchers at the end of each section, the loss has entry points of its own (ltu_loss_wide_*), whose arithmetic is that of
// loss.hip statement for statement (same four sums per (sample, class) {P, T, I, E}, same finalize, same coefficient form).
#include "manyclass.h"

static unsigned sgrid(long long n, int per_block = 256) {
  long long blocks = (n + per_block - 1) / per_block;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
#define GRID_STRIDE(i, n) \
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

#define WIDE_DISPATCH_C(C, ...)                              \
  do {                                                       \
    switch (C) {                                             \
      case 5: { constexpr int CT = 5; __VA_ARGS__ } break;   \
      case 6: { constexpr int CT = 6; __VA_ARGS__ } break;   \
      case 7: { constexpr int CT = 7; __VA_ARGS__ } break;   \
      case 8: { constexpr int CT = 8; __VA_ARGS__ } break;   \
      default: return LTU_E_SHAPE;                           \
    }                                                        \
  } while (0)

// a row of C fp32 values at a stride of 4 C bytes, with the widest access that stride keeps aligned (16 bytes for C = 8, 8 for
// C = 6, 4 for odd C); v[c >= C] = 0
template <int C>
__device__ __forceinline__ void ldrow(const float* __restrict__ q, float (&v)[8]) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int k = 0; k < C; k += 4) {
      const float4 t = *reinterpret_cast<const float4*>(q + k);
      v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
    }
  } else if constexpr (C % 2 == 0) {
#pragma unroll
    for (int k = 0; k < C; k += 2) {
      const float2 t = *reinterpret_cast<const float2*>(q + k);
      v[k] = t.x; v[k + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = q[k];
  }
#pragma unroll
  for (int k = C; k < 8; ++k) v[k] = 0.f;
}
template <int C>
__device__ __forceinline__ void strow(float* __restrict__ q, const float (&v)[8]) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int k = 0; k < C; k += 4) *reinterpret_cast<float4*>(q + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
  } else if constexpr (C % 2 == 0) {
#pragma unroll
    for (int k = 0; k < C; k += 2) *reinterpret_cast<float2*>(q + k) = make_float2(v[k], v[k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) q[k] = v[k];
  }
}
// the first 8 logits of a padded row: two 16-byte loads (fp32) or one (bf16)
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ q, float (&v)[8]);
template <>
__device__ __forceinline__ void load8<float>(const float* __restrict__ q, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <>
__device__ __forceinline__ void load8<bf16_t>(const bf16_t* __restrict__ q, float (&v)[8]) {
  const uint4 r = *reinterpret_cast<const uint4*>(q);
  v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
  v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
  v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
  v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}

// ------------------------------------------------------------------------------------------------ mask head
// logits T [M][CP] (first C live) -> probs f32 [M][C].  VEC: the row start is 16-byte aligned and holds >= 8 columns
template <typename T, int C, bool VEC>
__global__ void __launch_bounds__(256) head_softmax_wide_fwd_kernel(const T* __restrict__ z, float* __restrict__ p, long long M, int CP) {
  GRID_STRIDE(m, M) {
    float v[8];
    if constexpr (VEC) load8<T>(z + m * CP, v);
    else {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = ld1<T>(z + m * CP + c);
    }
    float mx = -INFINITY, sum = 0.f, r[8];
#pragma unroll
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - mx); sum += v[c]; }
#pragma unroll
    for (int c = 0; c < 8; ++c) r[c] = c < C ? v[c] / sum : 0.f;
    strow<C>(p + m * C, r);
  }
}
// g[c] = p_c (dp_c - sum_k dp_k p_k) for c < C, 0 behind
template <int C>
__device__ __forceinline__ void head_grad(const float* __restrict__ dp, const float* __restrict__ p, long long m, float (&g)[8]) {
  float a[8], b[8];
  ldrow<C>(dp + m * C, a);
  ldrow<C>(p + m * C, b);
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) dot += a[c] * b[c];
#pragma unroll
  for (int c = 0; c < 8; ++c) g[c] = c < C ? b[c] * (a[c] - dot) : 0.f;
}
// bf16 rows of CP = 8k padded logits: one thread and one 16-byte store per 8 columns, all four words of the first group live
template <int C>
__global__ void __launch_bounds__(256) head_softmax_wide_bwd_bf16x8_kernel(const float* __restrict__ dp, const float* __restrict__ p,
                                                                           uint4* __restrict__ dz, long long M, int CP) {
  const int v8 = CP / 8;
  GRID_STRIDE(i, M * v8) {
    const long long m = i / v8;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (i - m * v8 == 0) {
      float g[8];
      head_grad<C>(dp, p, m, g);
      o.x = pack_bf16x2(g[0], g[1]);
      o.y = pack_bf16x2(g[2], g[3]);
      o.z = pack_bf16x2(g[4], g[5]);
      o.w = pack_bf16x2(g[6], g[7]);
    }
    dz[i] = o;
  }
}
// one thread per row.  VEC: CP % 4 == 0 (so CP >= 8) and an aligned base: 4-wide stores, zeros behind the first 8 columns
template <typename T, int C, bool VEC>
__global__ void __launch_bounds__(256) head_softmax_wide_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ p, T* __restrict__ dz,
                                                                    long long M, int CP) {
  GRID_STRIDE(m, M) {
    float g[8];
    head_grad<C>(dp, p, m, g);
    T* o = dz + m * CP;
    if constexpr (VEC) {
      Vec4<T>::store(o, make_float4(g[0], g[1], g[2], g[3]));
      Vec4<T>::store(o + 4, make_float4(g[4], g[5], g[6], g[7]));
      for (int k = 8; k < CP; k += 4) Vec4<T>::store(o + k, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) st1<T>(o + c, g[c]);
      for (int c = C; c < CP; ++c) st1<T>(o + c, 0.f);
    }
  }
}
int ltu_head_softmax_wide_fwd(const void* z, float* p, long long M, int C, int CP, int dtype, ltu_stream_t s) {
  if (C < 5 || C > LTU_WIDE_MAXC || CP < C) return LTU_E_SHAPE;
  LTU_DISPATCH_T(dtype, {
    const bool vec = CP % (16 / (int)sizeof(T)) == 0 && ((uintptr_t)z & 15) == 0;
    WIDE_DISPATCH_C(C, {
      if (vec) hipLaunchKernelGGL((head_softmax_wide_fwd_kernel<T, CT, true>), dim3(sgrid(M)), dim3(256), 0, (hipStream_t)s, (const T*)z, p, M, CP);
      else hipLaunchKernelGGL((head_softmax_wide_fwd_kernel<T, CT, false>), dim3(sgrid(M)), dim3(256), 0, (hipStream_t)s, (const T*)z, p, M, CP);
    });
  });
  return ltu_check_launch();
}
int ltu_head_softmax_wide_bwd(const float* dp, const float* p, void* dz, long long M, int C, int CP, int dtype, ltu_stream_t s) {
  if (C < 5 || C > LTU_WIDE_MAXC || CP < C) return LTU_E_SHAPE;
  if (dtype == LTU_BF16 && CP % 8 == 0 && ((uintptr_t)dz & 15) == 0) {
    WIDE_DISPATCH_C(C, {
      hipLaunchKernelGGL(head_softmax_wide_bwd_bf16x8_kernel<CT>, dim3(sgrid(M * (CP / 8))), dim3(256), 0, (hipStream_t)s, dp, p, (uint4*)dz, M, CP);
    });
    return ltu_check_launch();
  }
  LTU_DISPATCH_T(dtype, {
    const bool vec = CP % 4 == 0 && ((uintptr_t)dz & 15) == 0;
    WIDE_DISPATCH_C(C, {
      if (vec) hipLaunchKernelGGL((head_softmax_wide_bwd_kernel<T, CT, true>), dim3(sgrid(M)), dim3(256), 0, (hipStream_t)s, dp, p, (T*)dz, M, CP);
      else hipLaunchKernelGGL((head_softmax_wide_bwd_kernel<T, CT, false>), dim3(sgrid(M)), dim3(256), 0, (hipStream_t)s, dp, p, (T*)dz, M, CP);
    });
  });
  return ltu_check_launch();
}

// ------------------------------------------------------------------------------------------------ final head
// z T [B,h,w,D,CP >= 4C] -> probs f32 [B,2h,2w,D,C]; channel c*4 + kh*2 + kw of coarse voxel (h,w) is class c of fine voxel
// (2h+kh, 2w+kw), so the 4-wide load at channel 4c is class c of the four fine voxels.  One thread per coarse voxel.
template <typename T, int C>
__global__ void __launch_bounds__(256) final_softmax_wide_fwd_kernel(const T* __restrict__ z, float* __restrict__ p, int B, int h, int w, int D, int CP) {
  const long long n = (long long)B * h * w * D;
  GRID_STRIDE(i, n) {
    const int d = (int)(i % D);
    long long t = i / D;
    const int ww = (int)(t % w); t /= w;
    const int hh = (int)(t % h);
    const int b = (int)(t / h);
    float4 v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = Vec4<T>::load(z + i * CP + 4 * c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float mx = -INFINITY, sum = 0.f, e[8], r[8];
#pragma unroll
      for (int c = 0; c < C; ++c) { e[c] = q == 0 ? v[c].x : q == 1 ? v[c].y : q == 2 ? v[c].z : v[c].w; mx = fmaxf(mx, e[c]); }
#pragma unroll
      for (int c = 0; c < C; ++c) { e[c] = expf(e[c] - mx); sum += e[c]; }
#pragma unroll
      for (int c = 0; c < 8; ++c) r[c] = c < C ? e[c] / sum : 0.f;
      strow<C>(p + ((((long long)b * 2 * h + 2 * hh + (q >> 1)) * 2 * w + 2 * ww + (q & 1)) * D + d) * C, r);
    }
  }
}
template <typename T, int C>
__global__ void __launch_bounds__(256) final_softmax_wide_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ p, T* __restrict__ dz,
                                                                     int B, int h, int w, int D, int CP) {
  const long long n = (long long)B * h * w * D;
  GRID_STRIDE(i, n) {
    const int d = (int)(i % D);
    long long t = i / D;
    const int ww = (int)(t % w); t /= w;
    const int hh = (int)(t % h);
    const int b = (int)(t / h);
    float gv[4][8], pv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                 // all loads of the four fine voxels first
      const long long o = ((((long long)b * 2 * h + 2 * hh + (q >> 1)) * 2 * w + 2 * ww + (q & 1)) * D + d) * C;
      ldrow<C>(dp + o, gv[q]);
      ldrow<C>(p + o, pv[q]);
    }
    float dot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      dot[q] = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) dot[q] += gv[q][c] * pv[q][c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      Vec4<T>::store(dz + i * CP + 4 * c, make_float4(pv[0][c] * (gv[0][c] - dot[0]), pv[1][c] * (gv[1][c] - dot[1]),
                                                      pv[2][c] * (gv[2][c] - dot[2]), pv[3][c] * (gv[3][c] - dot[3])));
    for (int k = 4 * C; k < CP; k += 4) Vec4<T>::store(dz + i * CP + k, make_float4(0.f, 0.f, 0.f, 0.f));      // padded conv columns
  }
}
int ltu_final_softmax_wide_fwd(const void* z, float* p, int B, int h, int w, int D, int C, int CP, int dtype, ltu_stream_t s) {
  if (C < 5 || C > LTU_WIDE_MAXC || CP < 4 * C || CP % 4) return LTU_E_SHAPE;
  LTU_DISPATCH_T(dtype, {
    const dim3 grid(sgrid((long long)B * h * w * D));
    WIDE_DISPATCH_C(C, { hipLaunchKernelGGL((final_softmax_wide_fwd_kernel<T, CT>), grid, dim3(256), 0, (hipStream_t)s, (const T*)z, p, B, h, w, D, CP); });
  });
  return ltu_check_launch();
}
int ltu_final_softmax_wide_bwd(const float* dp, const float* p, void* dz, int B, int h, int w, int D, int C, int CP, int dtype,
                               ltu_stream_t s) {
  if (C < 5 || C > LTU_WIDE_MAXC || CP < 4 * C || CP % 4) return LTU_E_SHAPE;
  LTU_DISPATCH_T(dtype, {
    const dim3 grid(sgrid((long long)B * h * w * D));
    WIDE_DISPATCH_C(C, { hipLaunchKernelGGL((final_softmax_wide_bwd_kernel<T, CT>), grid, dim3(256), 0, (hipStream_t)s, dp, p, (T*)dz, B, h, w, D, CP); });
  });
  return ltu_check_launch();
}

// ------------------------------------------------------------------------------------------------ level loss, 2 <= C <= 8
// Four voxels per thread and trip (S % 4 == 0): one 4-byte label load and C 16-byte probability loads.  Trips in flight: two
// up to C = 4 (the geometry of loss.hip), one above (4 C floats a trip: two trips of C = 8 would hold 64 loaded values beside
// the 32 accumulators).
template <int C>
__global__ void __launch_bounds__(256) loss_wide_sums_v4_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ sums,
                                                                long long S, int rows_per_block) {
  __shared__ float red[4][C * 4];
  const int b = blockIdx.y;
  float acc[C][4];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[c][k] = 0.f;
  const long long s0 = (long long)blockIdx.x * rows_per_block;
  long long s1 = s0 + rows_per_block;
  if (s1 > S) s1 = S;
  auto fetch = [&](long long s, uint32_t& labs, float (&f)[4 * C]) {
    labs = *reinterpret_cast<const uint32_t*>(label + (long long)b * S + s);
    const float* pv = p + ((long long)b * S + s) * C;
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const float4 t = *reinterpret_cast<const float4*>(pv + 4 * q);
      f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
    }
  };
  auto add = [&](uint32_t labs, const float (&f)[4 * C]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lab = (int)((labs >> (8 * j)) & 255u);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float pc = f[j * C + c];
        const float t = lab == c ? 1.f : 0.f;
        acc[c][0] += pc;
        acc[c][1] += t;
        acc[c][2] += pc * t;
        acc[c][3] += t * (1.f - pc) * logf(fmaxf(pc, 1e-6f));
      }
    }
  };
  long long s = s0 + (long long)threadIdx.x * 4;
  if constexpr (C <= 4) {
    for (; s + 1024 < s1; s += 2048) {
      uint32_t l0, l1;
      float f0[4 * C], f1[4 * C];
      fetch(s, l0, f0);
      fetch(s + 1024, l1, f1);
      add(l0, f0);
      add(l1, f1);
    }
    if (s < s1) {
      uint32_t l0;
      float f0[4 * C];
      fetch(s, l0, f0);
      add(l0, f0);
    }
  } else {
    for (; s < s1; s += 1024) {
      uint32_t l0;
      float f0[4 * C];
      fetch(s, l0, f0);
      add(l0, f0);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = wave_sum(acc[c][k]);
      if (lane == 0) red[wave][c * 4 + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < C * 4) {
    float v = 0.f;
    for (int w = 0; w < 4; ++w) v += red[w][threadIdx.x];
    // per-block partial [block][b][C*4] behind the final sums: folded by the finalize kernel in a fixed order, no fp32 atomics
    sums[((long long)(1 + blockIdx.x) * gridDim.y + b) * C * 4 + threadIdx.x] = v;
  }
}
// any S: one voxel per thread and trip
template <int C>
__global__ void __launch_bounds__(256) loss_wide_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ sums,
                                                             long long S, int rows_per_block) {
  __shared__ float red[4][C * 4];
  const int b = blockIdx.y;
  float acc[C][4];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[c][k] = 0.f;
  const long long s0 = (long long)blockIdx.x * rows_per_block;
  long long s1 = s0 + rows_per_block;
  if (s1 > S) s1 = S;
  for (long long s = s0 + threadIdx.x; s < s1; s += 256) {
    const int lab = label[(long long)b * S + s];
    const float* pv = p + ((long long)b * S + s) * C;
    float f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) f[c] = pv[c];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float pc = f[c];
      const float t = lab == c ? 1.f : 0.f;
      acc[c][0] += pc;
      acc[c][1] += t;
      acc[c][2] += pc * t;
      acc[c][3] += t * (1.f - pc) * logf(fmaxf(pc, 1e-6f));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = wave_sum(acc[c][k]);
      if (lane == 0) red[wave][c * 4 + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < C * 4) {
    float v = 0.f;
    for (int w = 0; w < 4; ++w) v += red[w][threadIdx.x];
    sums[((long long)(1 + blockIdx.x) * gridDim.y + b) * C * 4 + threadIdx.x] = v;
  }
}

// weights: w_ce, w_bal, w_dice[c] (standard per-class Dice on class c), w_fg (foreground union).  values out (C + 5 floats):
// [0] = total, [1] = ce, [2] = bal, [3 + c] = dice_c, [3 + C] = foreground-union dice, [4 + C] = total again.
// coef [B][C][3] = alpha, beta, gamma (already multiplied by the loss weights).
struct LossWideCfg {
  float w_ce, w_bal, w_dice[LTU_WIDE_MAXC], w_fg;
};

// the finalize of loss.hip with the class loops unrolled (compile-time C: the per-class arrays stay in registers).  Where a
// product meets a sum the fusing is written out, not left to -ffp-contract=fast: the compiler fuses every such site of
// loss.hip's rolled class loops but one (the first two terms of the total), while over the unrolled loops here it packs pairs of
// products into v_pk_mul_f32 and adds them unfused, and the CE value and the total then differ from ltu_loss_fwd's in the last bit.
template <int C>
__global__ void __launch_bounds__(256) loss_wide_finalize_kernel(float* __restrict__ sums, int nblk, float* __restrict__ values, float* __restrict__ coef,
                                                                 int B, long long S, LossWideCfg cfg, const float* __restrict__ scale_dev) {
#pragma clang fp contract(off)
  {
    // fold the per-block partials in a fixed order: output o = tid % nout is shared by the 256 / nout thread groups (each sums
    // every ngrp-th block, 8 loads in flight), which meet in LDS
    __shared__ float fold[256];
    const int nout = B * C * 4;                          // <= 256
    const int ngrp = 256 / nout;
    const int o = threadIdx.x % nout, grp = threadIdx.x / nout;
    float a0 = 0.f, a1 = 0.f;
    if (grp < ngrp) {
      const float* pp = sums + nout + o;
      int z = grp;
      for (; z + 7 * ngrp < nblk; z += 8 * ngrp) {
        const float v0 = pp[(long long)z * nout], v1 = pp[(long long)(z + ngrp) * nout], v2 = pp[(long long)(z + 2 * ngrp) * nout],
                    v3 = pp[(long long)(z + 3 * ngrp) * nout], v4 = pp[(long long)(z + 4 * ngrp) * nout],
                    v5 = pp[(long long)(z + 5 * ngrp) * nout], v6 = pp[(long long)(z + 6 * ngrp) * nout],
                    v7 = pp[(long long)(z + 7 * ngrp) * nout];
        a0 += (v0 + v1) + (v2 + v3); a1 += (v4 + v5) + (v6 + v7);
      }
      for (; z < nblk; z += ngrp) a0 += pp[(long long)z * nout];
    }
    fold[threadIdx.x] = a0 + a1;
    __syncthreads();
    if ((int)threadIdx.x < nout) {
      float t = 0.f;
      for (int g = 0; g < ngrp; ++g) t += fold[g * nout + threadIdx.x];
      sums[threadIdx.x] = t;
    }
    __syncthreads();
  }
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
  float total = cfg.w_ce * ce + cfg.w_bal * bal;          // two products and a sum, as loss.hip compiles it
  values[1] = ce;
  values[2] = bal;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float dv = 1.f - dice[c] / (float)B;
    values[3 + c] = dv;
    total = fmaf(cfg.w_dice[c], dv, total);
  }
  const float fgv = 1.f - fg / (float)B;
  values[3 + C] = fgv;
  total = fmaf(cfg.w_fg, fgv, total);
  values[0] = total;
  values[4 + C] = total;      // a second copy: the autograd wrapper exposes it as the differentiable scalar and the rest as the report
}

// dp[s,c] = gscale * (alpha + t (beta + gamma f'(p))); four voxels per thread (S % 4 == 0): 16-byte loads and stores
template <int C>
__global__ void __launch_bounds__(256) loss_wide_bwd_v4_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label,
                                                               const float* __restrict__ coef, const float* __restrict__ gscale,
                                                               float* __restrict__ dp, long long S) {
  const int b = blockIdx.y;
  const float gs = gscale[0];
  float k0[C], k1[C], k2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* k = coef + ((long long)b * C + c) * 3;
    k0[c] = k[0]; k1[c] = k[1]; k2[c] = k[2];
  }
  for (long long s = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; s < S; s += (long long)gridDim.x * 1024) {
    const long long i = (long long)b * S + s;
    const uint32_t labs = *reinterpret_cast<const uint32_t*>(label + i);
    float f[4 * C], o[4 * C];
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const float4 t = *reinterpret_cast<const float4*>(p + i * C + 4 * q);
      f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lab = (int)((labs >> (8 * j)) & 255u);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float pc = f[j * C + c];
        const float fp = -logf(fmaxf(pc, 1e-6f)) + (pc > 1e-6f ? (1.f - pc) / pc : 0.f);
        o[j * C + c] = gs * (lab == c ? k0[c] + (k1[c] + k2[c] * fp) : k0[c]);
      }
    }
#pragma unroll
    for (int q = 0; q < C; ++q) *reinterpret_cast<float4*>(dp + i * C + 4 * q) = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
  }
}
// any S: one voxel per thread and trip
template <int C>
__global__ void __launch_bounds__(256) loss_wide_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ label,
                                                            const float* __restrict__ coef, const float* __restrict__ gscale,
                                                            float* __restrict__ dp, long long S) {
  const int b = blockIdx.y;
  const float gs = gscale[0];
  float k0[C], k1[C], k2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* k = coef + ((long long)b * C + c) * 3;
    k0[c] = k[0]; k1[c] = k[1]; k2[c] = k[2];
  }
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < S; s += (long long)gridDim.x * 256) {
    const long long i = (long long)b * S + s;
    const int lab = label[i];
    float f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) f[c] = p[i * C + c];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float pc = f[c];
      const float fp = -logf(fmaxf(pc, 1e-6f)) + (pc > 1e-6f ? (1.f - pc) / pc : 0.f);
      dp[i * C + c] = gs * (lab == c ? k0[c] + (k1[c] + k2[c] * fp) : k0[c]);
    }
  }
}

// block geometry of the sums pass: that of ltu_loss_fwd
static long long loss_wide_rows(int B, long long S) {
  long long want = 1024 / (B > 0 ? B : 1);
  if (want < 1) want = 1;
  long long rows = (S + want - 1) / want;
  if (rows < 256) rows = 256;
  return (rows + 3) / 4 * 4;
}
static bool loss_wide_shape_ok(int B, long long S, int C) {
  return C >= 2 && C <= LTU_WIDE_MAXC && B >= 1 && S >= 1 && (long long)B * C * 4 <= 256;
}
extern "C" long long ltu_loss_wide_ws_floats(int B, long long S, int C) {
  if (!loss_wide_shape_ok(B, S, C)) return 0;
  return (1 + cdiv(S, loss_wide_rows(B, S))) * (long long)B * C * 4;
}

#define LOSS_WIDE_DISPATCH_C(C, ...)                         \
  do {                                                       \
    switch (C) {                                             \
      case 2: { constexpr int CT = 2; __VA_ARGS__ } break;   \
      case 3: { constexpr int CT = 3; __VA_ARGS__ } break;   \
      case 4: { constexpr int CT = 4; __VA_ARGS__ } break;   \
      case 5: { constexpr int CT = 5; __VA_ARGS__ } break;   \
      case 6: { constexpr int CT = 6; __VA_ARGS__ } break;   \
      case 7: { constexpr int CT = 7; __VA_ARGS__ } break;   \
      case 8: { constexpr int CT = 8; __VA_ARGS__ } break;   \
      default: return LTU_E_SHAPE;                           \
    }                                                        \
  } while (0)

extern "C" int ltu_loss_wide_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B,
                                 long long S, int C, float w_ce, float w_bal, const float* w_dice, const float* scale_dev, ltu_stream_t s) {
  if (!loss_wide_shape_ok(B, S, C)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || sums == nullptr || values == nullptr || coef == nullptr || w_dice == nullptr) return LTU_E_ARG;
  const long long rows = loss_wide_rows(B, S);
  const int nblk = (int)cdiv(S, rows);
  if ((1 + (long long)nblk) * B * C * 4 > sums_floats) return LTU_E_ARG;          // the scratch is shorter than this geometry needs
  LossWideCfg cfg;
  cfg.w_ce = w_ce; cfg.w_bal = w_bal;
  for (int c = 0; c < LTU_WIDE_MAXC; ++c) cfg.w_dice[c] = c < C ? w_dice[c] : 0.f;
  cfg.w_fg = w_dice[C];
  const bool v4 = S % 4 == 0 && !ltu_knob("LTU_LOSS_SCALAR", 0);
  LOSS_WIDE_DISPATCH_C(C, {
    if (v4) hipLaunchKernelGGL(loss_wide_sums_v4_kernel<CT>, dim3(nblk, B), dim3(256), 0, (hipStream_t)s, p, label, sums, S, (int)rows);
    else hipLaunchKernelGGL(loss_wide_sums_kernel<CT>, dim3(nblk, B), dim3(256), 0, (hipStream_t)s, p, label, sums, S, (int)rows);
    hipLaunchKernelGGL(loss_wide_finalize_kernel<CT>, dim3(1), dim3(256), 0, (hipStream_t)s, sums, nblk, values, coef, B, S, cfg, scale_dev);
  });
  return ltu_check_launch();
}

extern "C" int ltu_loss_wide_bwd(const float* p, const uint8_t* label, const float* coef, const float* gscale, float* dp, int B, long long S,
                                 int C, ltu_stream_t s) {
  if (!loss_wide_shape_ok(B, S, C)) return LTU_E_SHAPE;
  if (p == nullptr || label == nullptr || coef == nullptr || gscale == nullptr || dp == nullptr) return LTU_E_ARG;
  const bool v4 = S % 4 == 0 && !ltu_knob("LTU_LOSS_SCALAR", 0);
  const long long per = v4 ? 4 : 1;
  long long bx = (S / per + 255) / 256;
  const long long cap = 4096 / B > 1 ? 4096 / B : 1;
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  const dim3 grid((unsigned)bx, B);
  LOSS_WIDE_DISPATCH_C(C, {
    if (v4) hipLaunchKernelGGL(loss_wide_bwd_v4_kernel<CT>, grid, dim3(256), 0, (hipStream_t)s, p, label, coef, gscale, dp, S);
    else hipLaunchKernelGGL(loss_wide_bwd_kernel<CT>, grid, dim3(256), 0, (hipStream_t)s, p, label, coef, gscale, dp, S);
  });
  return ltu_check_launch();
}
