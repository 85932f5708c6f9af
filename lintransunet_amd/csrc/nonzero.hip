// Nonzero cropping and masked normalisation of a stored scan (data side; nnU-Net's crop_to_nonzero and ZScoreNormalization with
// use_mask_for_norm, which it runs on host copies; no reference counterpart).  Four streaming kernels around the hole filling of
// components.hip:
//   nz_mask_kernel       mask[i] = (accumulate ? mask[i] : 0) | (fmaf(v, slope, inter) != 0) over n voxels as stored (u8 / i16 /
//                        f32): one call per channel ORs the channels together.  A NaN is nonzero, -0.0 is zero.  A lane takes 16
//                        voxels: one 16-byte chunk of the mask, 1 / 2 / 4 of the image.  The chunks start at the mask's first
//                        16-byte boundary; the voxels before it (at most 15) and those after the last whole chunk go one by one,
//                        and an image that is not 16-byte aligned at that boundary is read element by element.
//   nz_box_kernel        bounding box and count of the set voxels of mask [B][H][W][D]: per lane 16 voxels, min / max / count along
//                        the wave, LDS atomics per workgroup, then one integer atomic per workgroup and bound (the reduction of
//                        surface.hip's box).  nz_box_init_kernel writes the empty box (lo = extent, hi = -1) and count 0 first.
//   nz_normalize_kernel  out[z][y][x] = mask ? fmaf(v, alpha, beta) : 0 over the box (lo, size) of the stored volume [S2][S1][S0]:
//                        the crop, the intensity map and the zeroing outside the mask in one pass; a lane writes 4 voxels.
// Integer atomics only (min, max, add commute): two calls give the same bytes.  Voxels beyond n / the box are never loaded.
// Nothing is allocated or synchronised: capturable.
#include "common.h"

#define NZ_THREADS 256
#define NZ_MAX_VOXELS 0xffffffffLL
#define NZ_INT_MAX 0x7fffffff

template <int DT>
__device__ __forceinline__ float nz_value(const void* __restrict__ img, long long i) {
  if (DT == LTU_U8) return (float)static_cast<const uint8_t*>(img)[i];
  if (DT == LTU_I16) return (float)static_cast<const int16_t*>(img)[i];
  return static_cast<const float*>(img)[i];
}

static int nz_elem_bytes(int dtype) { return dtype == LTU_U8 ? 1 : dtype == LTU_I16 ? 2 : dtype == LTU_F32 ? 4 : 0; }

// the 16 voxels from off on (all below n); vec: img + off is 16-byte aligned
template <int DT>
__device__ __forceinline__ void nz_load16(const void* __restrict__ img, long long off, bool vec, float v[16]) {
  if (!vec) {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = nz_value<DT>(img, off + k);
    return;
  }
  if (DT == LTU_U8) {
    const uint4 q = *reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(img) + off);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
  } else if (DT == LTU_I16) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint4 q = *reinterpret_cast<const uint4*>(static_cast<const int16_t*>(img) + off + 8 * j);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 8; ++k) v[8 * j + k] = (float)(int16_t)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 q = *reinterpret_cast<const float4*>(static_cast<const float*>(img) + off + 4 * j);
      v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
    }
  }
}

template <int DT>
__device__ __forceinline__ void nz_mask_one(const void* __restrict__ img, long long i, float slope, float inter, uint8_t* mask, int acc) {
  const uint8_t bit = fmaf(nz_value<DT>(img, i), slope, inter) != 0.f ? 1 : 0;
  mask[i] = acc ? (uint8_t)(mask[i] | bit) : bit;
}

// head: the voxels before the mask's first 16-byte boundary (< 16, <= n); chunk c covers [head + 16 c, head + 16 c + 16)
template <int DT>
__global__ void __launch_bounds__(NZ_THREADS) nz_mask_kernel(const void* __restrict__ img, long long n, float slope, float inter,
                                                             uint8_t* mask, int acc, int head, int vec) {
  const long long c = (long long)blockIdx.x * NZ_THREADS + threadIdx.x;
  if (c < head) nz_mask_one<DT>(img, c, slope, inter, mask, acc);
  const long long off = head + c * 16;
  if (off >= n) return;
  if (off + 16 > n) {
    for (long long i = off; i < n; ++i) nz_mask_one<DT>(img, i, slope, inter, mask, acc);
    return;
  }
  float v[16];
  nz_load16<DT>(img, off, vec != 0, v);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 16; ++k) w[k >> 2] |= (fmaf(v[k], slope, inter) != 0.f ? 1u : 0u) << (8 * (k & 3));
  uint4* m = reinterpret_cast<uint4*>(mask + off);
  if (acc) {
    const uint4 o = *m;
    w[0] |= o.x; w[1] |= o.y; w[2] |= o.z; w[3] |= o.w;
  }
  *m = make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DT>
static void nz_mask_launch(const void* img, long long n, float slope, float inter, uint8_t* mask, int acc, hipStream_t st) {
  long long head = (16 - (long long)((uintptr_t)mask & 15)) & 15;
  if (head > n) head = n;
  const int vec = (((uintptr_t)img + (uintptr_t)(head * nz_elem_bytes(DT))) & 15) == 0;
  const long long chunks = (n - head + 15) / 16;
  const long long lanes = chunks > head ? chunks : head;
  hipLaunchKernelGGL(nz_mask_kernel<DT>, dim3(cdiv(lanes, NZ_THREADS)), dim3(NZ_THREADS), 0, st, img, n, slope, inter, mask, acc,
                     (int)head, vec);
}

extern "C" int ltu_nonzero_mask(const void* img, int dtype, long long n_voxels, float slope, float inter, uint8_t* mask, int accumulate,
                                ltu_stream_t s) {
  const int es = nz_elem_bytes(dtype);
  if (es == 0) return LTU_E_DTYPE;
  if (n_voxels < 1 || n_voxels > NZ_MAX_VOXELS) return LTU_E_SHAPE;
  if (img == nullptr || mask == nullptr) return LTU_E_ARG;
  if (((uintptr_t)img & (uintptr_t)(es - 1)) != 0) return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  const int acc = accumulate != 0;
  if (dtype == LTU_U8) nz_mask_launch<LTU_U8>(img, n_voxels, slope, inter, mask, acc, st);
  else if (dtype == LTU_I16) nz_mask_launch<LTU_I16>(img, n_voxels, slope, inter, mask, acc, st);
  else nz_mask_launch<LTU_F32>(img, n_voxels, slope, inter, mask, acc, st);
  return ltu_check_launch();
}

// ---- bounding box and count ------------------------------------------------------------------------------------------------
// box [B][6] = (h0, h1, w0, w1, d0, d1): the even slots hold minima, the odd ones maxima
__global__ void nz_box_init_kernel(int* __restrict__ box, unsigned long long* __restrict__ count, int B, int H, int W, int D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 6 * B) {
    const int a = (i % 6) >> 1;
    box[i] = (i & 1) ? -1 : (a == 0 ? H : a == 1 ? W : D);
  }
  if (i < B) count[i] = 0ull;
}

// grid = (runs of 256 x 16 voxels, B)
__global__ void __launch_bounds__(NZ_THREADS) nz_box_kernel(const uint8_t* __restrict__ mask, int* __restrict__ box,
                                                            unsigned long long* __restrict__ count, int H, int W, int D) {
  __shared__ int sb[6];
  __shared__ int scount;
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const long long S = (long long)H * W * D;
  const uint8_t* mb = mask + (long long)b * S;
  if (threadIdx.x < 6) sb[threadIdx.x] = (threadIdx.x & 1) ? -1 : NZ_INT_MAX;
  if (threadIdx.x == 6) scount = 0;
  __syncthreads();
  const long long v0 = ((long long)blockIdx.x * NZ_THREADS + threadIdx.x) * 16;
  int lo[3] = {NZ_INT_MAX, NZ_INT_MAX, NZ_INT_MAX}, hi[3] = {-1, -1, -1}, cnt = 0;
  if (v0 < S) {
    const int valid = v0 + 16 <= S ? 16 : (int)(S - v0);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (valid == 16 && ((uintptr_t)(mb + v0) & 15) == 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(mb + v0);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
      for (int k = 0; k < valid; ++k) w[k >> 2] |= (uint32_t)mb[v0 + k] << (8 * (k & 3));
    }
    if ((w[0] | w[1] | w[2] | w[3]) != 0u) {
      int c[3];                                   // (h, w, d) of voxel v0 + k, stepped along the raster
      c[2] = (int)(v0 % D);
      c[1] = (int)((v0 / D) % W);
      c[0] = (int)(v0 / ((long long)W * D));
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if ((w[k >> 2] >> (8 * (k & 3))) & 0xffu) {
          ++cnt;
#pragma unroll
          for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
        }
        if (++c[2] == D) {
          c[2] = 0;
          if (++c[1] == W) { c[1] = 0; ++c[0]; }
        }
      }
    }
  }
  if (__ballot(cnt > 0) != 0ull) {                // wave-uniform: most waves of a skull-stripped scan see zeros only
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o);
#pragma unroll
      for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], __shfl_xor(lo[a], o)); hi[a] = max(hi[a], __shfl_xor(hi[a], o)); }
    }
  }
  if (lane == 0 && cnt > 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&sb[2 * a], lo[a]); atomicMax(&sb[2 * a + 1], hi[a]); }
    atomicAdd(&scount, cnt);
  }
  __syncthreads();
  if (scount == 0) return;
  if (threadIdx.x < 6) {
    if (threadIdx.x & 1) atomicMax(box + 6 * b + threadIdx.x, sb[threadIdx.x]);
    else atomicMin(box + 6 * b + threadIdx.x, sb[threadIdx.x]);
  }
  if (threadIdx.x == 6) atomicAdd(&count[b], (unsigned long long)scount);
}

extern "C" int ltu_mask_box(const uint8_t* mask, int B, int H, int W, int D, int* box, unsigned long long* count, ltu_stream_t s) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || D < 1 || (long long)H * W * D >= (1LL << 31)) return LTU_E_SHAPE;
  if (mask == nullptr || box == nullptr || count == nullptr) return LTU_E_ARG;
  if (((uintptr_t)box & 3) != 0 || ((uintptr_t)count & 7) != 0) return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  hipLaunchKernelGGL(nz_box_init_kernel, dim3(cdiv(6LL * B, 256)), dim3(256), 0, st, box, count, B, H, W, D);
  hipLaunchKernelGGL(nz_box_kernel, dim3(cdiv(S, NZ_THREADS * 16), B), dim3(NZ_THREADS), 0, st, mask, box, count, H, W, D);
  return ltu_check_launch();
}

// ---- crop + masked intensity map -------------------------------------------------------------------------------------------
// out [n2][n1][n0] from the box (l0, l1, l2) + (n0, n1, n2) of img / mask [S2][S1][S0]; a lane writes out[o0 .. o0 + 4)
template <int DT>
__global__ void __launch_bounds__(NZ_THREADS) nz_normalize_kernel(const void* __restrict__ img, const uint8_t* __restrict__ mask,
                                                                  long long S0, long long S1, int l0, int l1, int l2, int n0, int n1,
                                                                  float alpha, float beta, float* __restrict__ out, long long total,
                                                                  int vec) {
  const long long o0 = ((long long)blockIdx.x * NZ_THREADS + threadIdx.x) * 4;
  if (o0 >= total) return;
  const int valid = o0 + 4 <= total ? 4 : (int)(total - o0);
  int x = (int)(o0 % n0), y = (int)((o0 / n0) % n1);
  long long z = o0 / ((long long)n0 * n1);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < valid) {
      const long long src = ((z + l2) * S1 + (y + l1)) * S0 + (x + l0);
      if (mask[src]) v[k] = fmaf(nz_value<DT>(img, src), alpha, beta);
      if (++x == n0) {
        x = 0;
        if (++y == n1) { y = 0; ++z; }
      }
    }
  }
  if (valid == 4 && vec) {
    *reinterpret_cast<float4*>(out + o0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < valid; ++k) out[o0 + k] = v[k];
  }
}

extern "C" int ltu_normalize_masked(const void* img, int dtype, const uint8_t* mask, int S0, int S1, int S2, int l0, int l1, int l2,
                                    int n0, int n1, int n2, float alpha, float beta, float* out, ltu_stream_t s) {
  const int es = nz_elem_bytes(dtype);
  if (es == 0) return LTU_E_DTYPE;
  if (S0 < 1 || S1 < 1 || S2 < 1 || (long long)S0 * S1 * S2 > NZ_MAX_VOXELS) return LTU_E_SHAPE;
  if (l0 < 0 || l1 < 0 || l2 < 0 || n0 < 1 || n1 < 1 || n2 < 1 || n0 > S0 - l0 || n1 > S1 - l1 || n2 > S2 - l2) return LTU_E_SHAPE;
  if (img == nullptr || mask == nullptr || out == nullptr) return LTU_E_ARG;
  if (((uintptr_t)img & (uintptr_t)(es - 1)) != 0 || ((uintptr_t)out & 3) != 0) return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  const long long total = (long long)n0 * n1 * n2;
  const int vec = ((uintptr_t)out & 15) == 0;
  const dim3 grid(cdiv(total, NZ_THREADS * 4)), block(NZ_THREADS);
  if (dtype == LTU_U8)
    hipLaunchKernelGGL(nz_normalize_kernel<LTU_U8>, grid, block, 0, st, img, mask, (long long)S0, (long long)S1, l0, l1, l2, n0, n1, alpha,
                       beta, out, total, vec);
  else if (dtype == LTU_I16)
    hipLaunchKernelGGL(nz_normalize_kernel<LTU_I16>, grid, block, 0, st, img, mask, (long long)S0, (long long)S1, l0, l1, l2, n0, n1, alpha,
                       beta, out, total, vec);
  else
    hipLaunchKernelGGL(nz_normalize_kernel<LTU_F32>, grid, block, 0, st, img, mask, (long long)S0, (long long)S1, l0, l1, l2, n0, n1, alpha,
                       beta, out, total, vec);
  return ltu_check_launch();
}
