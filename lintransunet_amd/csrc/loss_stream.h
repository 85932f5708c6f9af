// The streaming skeleton of the level-loss kernels (loss.hip, loss_ext.hip): how a block of 256 threads walks the voxels of a
// sample, how per-thread sums become per-block partials and how the finalize kernel folds those.  What a voxel adds to the sums and
// what its gradient is stays with each file, as a functor.  One definition each; no kernels here.
#pragma once
#include "common.h"

// four voxels from the flat voxel index i (a multiple of 4): one 4-byte label load and C 16-byte probability loads
template <int C>
__device__ __forceinline__ void ls_fetch4(const float* __restrict__ p, const uint8_t* __restrict__ label, long long i, uint32_t& labs,
                                          float (&f)[4 * C]) {
  labs = *reinterpret_cast<const uint32_t*>(label + i);
  const float* pv = p + i * C;
#pragma unroll
  for (int q = 0; q < C; ++q) {
    const float4 t = *reinterpret_cast<const float4*>(pv + 4 * q);
    f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
  }
}
// add(lab, f) for each of the four, in voxel order
template <int C, class Add>
__device__ __forceinline__ void ls_add4(uint32_t labs, const float (&f)[4 * C], Add& add) {
#pragma unroll
  for (int j = 0; j < 4; ++j) add((int)((labs >> (8 * j)) & 255u), f + j * C);
}

// A product that meets a sum as a value rounded on its own: passed through here it is not contracted into the sum (the contraction
// pragma does not reach the backend; see the finalize kernel of loss.hip)
__device__ __forceinline__ float ls_rounded(float v) {
  asm("" : "+v"(v));
  return v;
}

// Sums pass: block x walks voxels [x rows_per_block, (x + 1) rows_per_block) of sample blockIdx.y and calls add(lab, f[C]) per voxel.
// V4 (S % 4 == 0, C >= 2, rows_per_block % 4 == 0): four voxels per thread and trip; TWO: two trips in flight (4 C floats a trip: two
// trips of C = 8 would hold 64 loaded values beside the accumulators).  Otherwise one voxel per thread and trip (a 1-byte and C
// 4-byte loads, 16 dependent trips per thread at level 0: that pass ran at 2.2 TB/s).
template <int C, bool V4, bool TWO, class Add>
__device__ __forceinline__ void ls_walk_block(const float* __restrict__ p, const uint8_t* __restrict__ label, long long S, int rows_per_block,
                                              Add add) {
  const long long base = (long long)blockIdx.y * S;
  const long long s0 = (long long)blockIdx.x * rows_per_block;
  long long s1 = s0 + rows_per_block;
  if (s1 > S) s1 = S;
  if constexpr (V4) {
    long long s = s0 + (long long)threadIdx.x * 4;
    uint32_t l0, l1;
    if constexpr (TWO) {
      for (; s + 1024 < s1; s += 2048) {
        float f0[4 * C], f1[4 * C];
        ls_fetch4<C>(p, label, base + s, l0, f0);
        ls_fetch4<C>(p, label, base + s + 1024, l1, f1);
        ls_add4<C>(l0, f0, add);
        ls_add4<C>(l1, f1, add);
      }
      if (s < s1) {
        float f0[4 * C];
        ls_fetch4<C>(p, label, base + s, l0, f0);
        ls_add4<C>(l0, f0, add);
      }
    } else {
      for (; s < s1; s += 1024) {
        float f0[4 * C];
        ls_fetch4<C>(p, label, base + s, l0, f0);
        ls_add4<C>(l0, f0, add);
      }
    }
  } else {
    for (long long s = s0 + threadIdx.x; s < s1; s += 256) {
      const int lab = label[base + s];
      const float* pv = p + (base + s) * C;
      float f[C];
#pragma unroll
      for (int c = 0; c < C; ++c) f[c] = pv[c];
      add(lab, f);
    }
  }
}

// The block's W sums of sample b = blockIdx.y -> sums[(1 + block) * B + b][W]: wave sums, the four waves meet in LDS.  A per-block
// partial behind the final sums, folded by the finalize kernel in a fixed order (no fp32 atomics: their order, and with it the last
// bit of every loss coefficient, changed from run to run - bf16 rounding downstream turns that bit into 1e-2 of some gradients).
template <int W>
__device__ __forceinline__ void ls_store_partial(const float (&acc)[W], float* __restrict__ sums) {
  __shared__ float red[4][W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < W) {
    float v = 0.f;
    for (int w = 0; w < 4; ++w) v += red[w][threadIdx.x];
    sums[((long long)(1 + blockIdx.x) * gridDim.y + blockIdx.y) * W + threadIdx.x] = v;
  }
}

// Gradient pass: a grid-stride walk over the S voxels of sample blockIdx.y, grad(lab, f[C], o[C]) per voxel.  V4 (S % 4 == 0): four
// voxels per thread, 16-byte loads and stores; otherwise one.
template <int C, bool V4, class Grad>
__device__ __forceinline__ void ls_walk_grid(const float* __restrict__ p, const uint8_t* __restrict__ label, float* __restrict__ dp, long long S,
                                             Grad grad) {
  const long long base = (long long)blockIdx.y * S;
  if constexpr (V4) {
    for (long long s = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; s < S; s += (long long)gridDim.x * 1024) {
      const long long i = base + s;
      uint32_t labs;
      float f[4 * C], o[4 * C];
      ls_fetch4<C>(p, label, i, labs, f);
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
      for (int c = 0; c < C; ++c) f[c] = p[i * C + c];
      grad((int)label[i], f, o);
#pragma unroll
      for (int c = 0; c < C; ++c) dp[i * C + c] = o[c];
    }
  }
}

// Head of a finalize kernel (one block of 256 threads): the per-block partials sums[(1 + z) * nout + o], z < nblk, fold in a fixed
// order into out[o], o < nout <= 256.  Output o = tid % nout is shared by the 256 / nout thread groups (each sums every ngrp-th
// block, 8 loads in flight), which meet in LDS.  Additions only.  out may be the head of sums or LDS; ends on a barrier.
__device__ __forceinline__ void ls_fold(const float* sums, int nblk, int nout, float* out) {
  __shared__ float fold[256];
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
    out[threadIdx.x] = t;
  }
  __syncthreads();
}

// ---- host side
// the four-voxel kernels: S % 4 == 0 and at least two classes; LTU_LOSS_SCALAR forces one voxel per thread
static inline bool loss_v4(long long S, int C) { return S % 4 == 0 && C >= 2 && !ltu_knob("LTU_LOSS_SCALAR", 0); }
// grid of a gradient pass: a trip of every thread, at most 4096 blocks over the batch
static inline dim3 loss_bwd_grid(int B, long long S, bool v4) {
  const int nb = B > 0 ? B : 1;
  long long bx = (S / (v4 ? 4 : 1) + 255) / 256;
  const long long cap = 4096 / nb > 1 ? 4096 / nb : 1;
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  return dim3((unsigned)bx, B);
}
