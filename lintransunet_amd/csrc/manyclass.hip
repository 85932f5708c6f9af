// Training path for 5 .. 8 classes on gfx950: mask-head softmax and final head (window un-embedding + softmax), forward and
// backward.  The class count is a template argument everywhere: per-thread arrays are indexed by unrolled loops only (a run-time
// class loop over them would put them in scratch memory or serialise the loads, see the CT = 0 path of pointwise.hip), and all
// loads of a row / coarse voxel are issued before the arithmetic.
//
// C <= 4 keeps the kernels of pointwise.hip; ltu_head_softmax_* and ltu_final_softmax_* hand C = 5 .. 8 over to the launchers at
// the end of each section.  The level loss of every class count is in loss.hip.
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
