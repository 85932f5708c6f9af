// Intensity fingerprint of one stored scan (data side; nnU-Net's dataset fingerprint / CTNormalization statistics, which it takes
// with np.percentile over host copies).  The scan (u8 / i16 / f32, n voxels as stored), optionally under its u8 label, becomes
// an exact value histogram: a 16-bit key per selected voxel, counted into hist uint32[65536] in global memory.
//   selection: lab == NULL, or bit min(lab[i], 8) of mask_bits set (the bin sets of crop_index.hip)
//   key:       LTU_HIST_U8 v; LTU_HIST_I16 v + 32768; LTU_HIST_F32_INT (int)v + 32768 for an f32 holding an integer of the i16 range;
//              LTU_HIST_F32_HI / _LO the top / low 16 bits of the float's order-preserving key (sign set: all bits flipped, else the
//              sign bit set; -0.0 counts as +0.0), _LO only for the voxels whose top 16 bits equal `prefix`
//   counts:    u64 {voxels binned, voxels rejected}: a non-finite f32, or in F32_INT one that is no integer of the range
// intensity_hist_kernel: a workgroup owns a contiguous run of the scan; a lane takes 16 voxels per trip (one 16-byte chunk of the
//   label, 1 / 2 / 4 chunks of the image, fetched only when the wave selected something).  65536 bins do not fit LDS, a scan's values
//   do fit windows: the workgroup keeps IH_NWIN windows of IH_WIN bins in LDS, the first placed around the first selected key one of
//   its waves meets, each further one around the first key that misses those before it (an LDS compare-and-swap each, no barrier).
//   Air and tissue of a CT lie 1000 bins apart and share a window; the ordered keys of a float scan take one for the negative values,
//   one for the positive ones (32 binades each) and one for 0.0, which lies 127 binades from 1.0.  Keys outside all of them go to
//   global atomics, one address per lane: 42 000 zeros left outside cost 370 us on a 26 M-voxel scan, hence the spare windows.  Per voxel slot the wave ballots the lanes that
//   share its first lane's key and adds their count once (the hot bin: air, or the few dozen values under a label), the others add 1
//   each.  At the end one global add per non-empty LDS bin.
// intensity_moments_kernel / intensity_fold_kernel: sum (v - c) and sum (v - c)^2 of the selected finite f32 voxels in fp64, one pair
//   per workgroup in a fixed order, folded in index order by one thread: no floating-point atomics.
// Integer adds commute, every partial has a fixed order: two calls give the same bytes.  Voxels at or beyond n are neither loaded
// nor counted (a chunk that straddles n is read element by element below n).  Nothing is allocated or synchronised: capturable.
#include "common.h"

#define IH_THREADS 512
#define IH_MAX_BLOCKS 512                          // two workgroups per CU: every workgroup ends with one global add per live bin
#define IH_WIN 4096                                // bins of one LDS window
#define IH_NWIN 4                                  // windows per workgroup: 64 KiB of LDS
#define IH_NONE 0xffffffffu
#define IH_MAX_VOXELS 0xffffffffLL
#define IM_THREADS 256

static bool ih_size_ok(long long n) { return n >= 1 && n <= IH_MAX_VOXELS; }

__device__ __forceinline__ unsigned ih_selected(uint32_t labv, unsigned mask) { return (mask >> (labv < 8u ? labv : 8u)) & 1u; }

// bit k of the result: voxel off + k (k < 16, below n) is selected.  lab 16-byte aligned, off a multiple of 16.
__device__ __forceinline__ unsigned ih_select16(const uint8_t* __restrict__ lab, long long off, long long n, unsigned mask) {
  if (off >= n) return 0u;
  const int valid = off + 16 <= n ? 16 : (int)(n - off);
  if (lab == nullptr) return 0xffffu >> (16 - valid);
  unsigned sel = 0u;
  if (valid == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(lab + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) sel |= ih_selected((w[k >> 2] >> (8 * (k & 3))) & 0xffu, mask) << k;
  } else {
    for (int k = 0; k < valid; ++k) sel |= ih_selected(lab[off + k], mask) << k;
  }
  return sel;
}

// the 16 voxels from off on as raw words (u8, sign-extended i16, f32 bits); those at or beyond n stay 0 and are not loaded
template <int DT>
__device__ __forceinline__ void ih_load16(const void* __restrict__ img, long long off, long long n, uint32_t v[16]) {
  if (off + 16 <= n) {
    if (DT == LTU_U8) {
      const uint4 q = *reinterpret_cast<const uint4*>((const uint8_t*)img + off);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    } else if (DT == LTU_I16) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint4 q = *reinterpret_cast<const uint4*>((const int16_t*)img + off + 8 * j);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) v[8 * j + k] = (uint32_t)(int32_t)(int16_t)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 q = *reinterpret_cast<const uint4*>((const uint32_t*)img + off + 4 * j);
        v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
      }
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    v[k] = 0u;
    if (off + k < n) {
      if (DT == LTU_U8) v[k] = ((const uint8_t*)img)[off + k];
      else if (DT == LTU_I16) v[k] = (uint32_t)(int32_t)((const int16_t*)img)[off + k];
      else v[k] = ((const uint32_t*)img)[off + k];
    }
  }
}

// 0: binned under `key`; 1: rejected; 2: skipped (F32_LO outside the prefix)
template <int MODE>
__device__ __forceinline__ int ih_key(uint32_t raw, uint32_t prefix, uint32_t& key) {
  if (MODE == LTU_HIST_U8) { key = raw; return 0; }
  if (MODE == LTU_HIST_I16) { key = raw + 32768u; return 0; }
  if ((raw & 0x7f800000u) == 0x7f800000u) return 1;                 // Inf, NaN
  if (MODE == LTU_HIST_F32_INT) {
    const float f = __uint_as_float(raw);
    if (!(f >= -32768.f && f <= 32767.f) || f != truncf(f)) return 1;
    key = (uint32_t)((int)f + 32768);
    return 0;
  }
  if (raw == 0x80000000u) raw = 0u;
  const uint32_t ord = (raw & 0x80000000u) ? ~raw : (raw | 0x80000000u);
  if (MODE == LTU_HIST_F32_HI) { key = ord >> 16; return 0; }
  if ((ord >> 16) != prefix) return 2;
  key = ord & 0xffffu;
  return 0;
}

// the window of `slot` as this wave must use it: placed around `key` (the key of lane src) unless another wave has placed it
__device__ __forceinline__ uint32_t ih_place(uint32_t* slot, uint32_t key, int src, int lane) {
  uint32_t got = 0u;
  if (lane == src) {
    uint32_t want = key < IH_WIN / 2 ? 0u : (key - IH_WIN / 2) & ~63u;
    if (want > 65536u - IH_WIN) want = 65536u - IH_WIN;
    const uint32_t old = atomicCAS(slot, IH_NONE, want);
    got = old == IH_NONE ? want : old;
  }
  return (uint32_t)__builtin_amdgcn_readlane((int)got, src);
}

template <int DT, int MODE>
__global__ void __launch_bounds__(IH_THREADS) intensity_hist_kernel(const void* __restrict__ img, const uint8_t* __restrict__ lab,
                                                                    long long n, unsigned mask, uint32_t prefix,
                                                                    uint32_t* __restrict__ hist, unsigned long long* __restrict__ counts,
                                                                    long long trips_per_block) {
  __shared__ uint32_t h[IH_NWIN * IH_WIN];
  __shared__ uint32_t s_base[IH_NWIN];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int b = tid; b < IH_NWIN * IH_WIN; b += IH_THREADS) h[b] = 0u;
  if (tid < IH_NWIN) s_base[tid] = IH_NONE;
  __syncthreads();
  uint32_t base[IH_NWIN] = {};                     // wave-uniform copies of the windows this wave knows: base[0 .. nset)
  int nset = 0;
  uint32_t n_bin = 0u, n_rej = 0u;
  const long long trip0 = (long long)blockIdx.x * trips_per_block;
  for (long long t = trip0; t < trip0 + trips_per_block; ++t) {
    const long long off = (t * IH_THREADS + tid) * 16;
    if (t * IH_THREADS * 16 >= n) break;           // workgroup-uniform
    const unsigned sel = ih_select16(lab, off, n, mask);
    if (__ballot(sel != 0u) == 0ull) continue;     // wave-uniform: nothing of this wave's 1024 voxels is selected
    uint32_t v[16];
    if (sel != 0u) ih_load16<DT>(img, off, n, v);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      uint32_t key = 0u;
      const int what = ((sel >> k) & 1u) ? ih_key<MODE>(v[k], prefix, key) : 2;
      n_rej += what == 1;
      const bool live = what == 0;
      n_bin += live;
      const unsigned long long ml = __ballot(live);
      if (ml == 0ull) continue;                    // wave-uniform
      const int src = __ffsll((long long)ml) - 1;
      const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, src);
      int win = IH_NWIN;                           // the first known window that holds this lane's key
#pragma unroll
      for (int w = IH_NWIN - 1; w >= 0; --w)
        if (w < nset && key - base[w] < (uint32_t)IH_WIN) win = w;
      // wave-uniform: the next window goes around the first key that misses the known ones, until this slot's keys are all housed
      // (a key left outside is a global add on a line every workgroup adds to)
      while (nset < IH_NWIN) {
        const unsigned long long mm = __ballot(live && win == IH_NWIN);
        if (mm == 0ull) break;
        const int s1 = __ffsll((long long)mm) - 1;
        const uint32_t nb = ih_place(&s_base[nset], (uint32_t)__builtin_amdgcn_readlane((int)key, s1), s1, lane);
#pragma unroll
        for (int w = 0; w < IH_NWIN; ++w)
          if (w == nset) base[w] = nb;
        if (win == IH_NWIN && key - nb < (uint32_t)IH_WIN) win = nset;
        ++nset;
      }
      const bool same = live && key == k0;
      const uint32_t cnt = (uint32_t)__popcll(__ballot(same));
      const uint32_t add = lane == src ? cnt : 1u;
      if (lane == src || (live && !same)) {
        uint32_t wb = 0u;
#pragma unroll
        for (int w = 0; w < IH_NWIN; ++w)
          if (w == win) wb = base[w];
        if (win < IH_NWIN) atomicAdd(&h[win * IH_WIN + (key - wb)], add);
        else atomicAdd(&hist[key], add);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_bin += __shfl_xor(n_bin, o);
    n_rej += __shfl_xor(n_rej, o);
  }
  if (lane == 0) {
    if (n_bin) atomicAdd(&counts[0], (unsigned long long)n_bin);
    if (n_rej) atomicAdd(&counts[1], (unsigned long long)n_rej);
  }
  __syncthreads();
  for (int w = 0; w < IH_NWIN; ++w) {
    const uint32_t wb = s_base[w];
    if (wb == IH_NONE) break;                      // workgroup-uniform: the windows are placed in order
    for (int b = tid; b < IH_WIN; b += IH_THREADS) {
      const uint32_t c = h[w * IH_WIN + b];
      if (c) atomicAdd(&hist[wb + b], c);
    }
  }
}

// parts[2 * block] = sum (v - c), parts[2 * block + 1] = sum (v - c)^2 over the block's selected finite voxels
__global__ void __launch_bounds__(IM_THREADS) intensity_moments_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab,
                                                                       long long n, unsigned mask, double c, double* __restrict__ parts,
                                                                       long long trips_per_block) {
  __shared__ double red[2][IM_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s1 = 0.0, s2 = 0.0;
  const long long trip0 = (long long)blockIdx.x * trips_per_block;
  for (long long t = trip0; t < trip0 + trips_per_block; ++t) {
    const long long off = (t * IM_THREADS + tid) * 16;
    if (t * IM_THREADS * 16 >= n) break;
    const unsigned sel = ih_select16(lab, off, n, mask);
    if (sel == 0u) continue;
    uint32_t v[16];
    ih_load16<LTU_F32>(img, off, n, v);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (((sel >> k) & 1u) && (v[k] & 0x7f800000u) != 0x7f800000u) {
        const double d = (double)__uint_as_float(v[k]) - c;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {               // a fixed tree: the same bits in every lane and in every call
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < IM_THREADS / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    parts[2 * blockIdx.x] = a;
    parts[2 * blockIdx.x + 1] = b;
  }
}

__global__ void intensity_fold_kernel(const double* __restrict__ parts, int nblk, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < nblk; ++i) { a += parts[2 * i]; b += parts[2 * i + 1]; }
  out[0] = a;
  out[1] = b;
}

template <int DT, int MODE>
static void ih_launch(const void* img, const uint8_t* lab, long long n, unsigned mask, uint32_t prefix, uint32_t* hist,
                      unsigned long long* counts, hipStream_t st) {
  const long long trips = (n + IH_THREADS * 16 - 1) / (IH_THREADS * 16);
  const long long per = (trips + IH_MAX_BLOCKS - 1) / IH_MAX_BLOCKS;
  hipLaunchKernelGGL((intensity_hist_kernel<DT, MODE>), dim3(cdiv(trips, per)), dim3(IH_THREADS), 0, st, img, lab, n, mask, prefix, hist,
                     counts, per);
}

extern "C" int ltu_intensity_hist(const void* img, int dtype, const uint8_t* lab, long long n_voxels, int mask_bits, int mode, int prefix,
                                  uint32_t* hist, unsigned long long* counts, ltu_stream_t s) {
  if (!ih_size_ok(n_voxels)) return LTU_E_SHAPE;
  if (img == nullptr || hist == nullptr || counts == nullptr) return LTU_E_ARG;
  if (mask_bits < 0 || mask_bits > 0x1ff || prefix < 0 || prefix > 0xffff) return LTU_E_ARG;
  const bool pair = (dtype == LTU_U8 && mode == LTU_HIST_U8) || (dtype == LTU_I16 && mode == LTU_HIST_I16) ||
                    (dtype == LTU_F32 && (mode == LTU_HIST_F32_INT || mode == LTU_HIST_F32_HI || mode == LTU_HIST_F32_LO));
  if (!pair) return LTU_E_ARG;
  if (((uintptr_t)img & 15) != 0 || (lab != nullptr && ((uintptr_t)lab & 15) != 0) || ((uintptr_t)hist & 3) != 0 ||
      ((uintptr_t)counts & 7) != 0)
    return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  const unsigned mask = (unsigned)mask_bits;
  const uint32_t pre = (uint32_t)prefix;
  switch (mode) {
    case LTU_HIST_U8: ih_launch<LTU_U8, LTU_HIST_U8>(img, lab, n_voxels, mask, pre, hist, counts, st); break;
    case LTU_HIST_I16: ih_launch<LTU_I16, LTU_HIST_I16>(img, lab, n_voxels, mask, pre, hist, counts, st); break;
    case LTU_HIST_F32_INT: ih_launch<LTU_F32, LTU_HIST_F32_INT>(img, lab, n_voxels, mask, pre, hist, counts, st); break;
    case LTU_HIST_F32_HI: ih_launch<LTU_F32, LTU_HIST_F32_HI>(img, lab, n_voxels, mask, pre, hist, counts, st); break;
    default: ih_launch<LTU_F32, LTU_HIST_F32_LO>(img, lab, n_voxels, mask, pre, hist, counts, st); break;
  }
  return ltu_check_launch();
}

extern "C" int ltu_intensity_moments(const float* img, const uint8_t* lab, long long n_voxels, int mask_bits, double centre, double* parts,
                                     long long parts_elems, double* out, ltu_stream_t s) {
  if (!ih_size_ok(n_voxels)) return LTU_E_SHAPE;
  if (img == nullptr || parts == nullptr || out == nullptr || parts_elems < 2 * LTU_INTENSITY_MOMENT_PARTS) return LTU_E_ARG;
  if (mask_bits < 0 || mask_bits > 0x1ff || !(centre - centre == 0.0)) return LTU_E_ARG;
  if (((uintptr_t)img & 15) != 0 || (lab != nullptr && ((uintptr_t)lab & 15) != 0) || ((uintptr_t)parts & 7) != 0 ||
      ((uintptr_t)out & 7) != 0)
    return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  const long long trips = (n_voxels + IM_THREADS * 16 - 1) / (IM_THREADS * 16);
  const long long per = (trips + LTU_INTENSITY_MOMENT_PARTS - 1) / LTU_INTENSITY_MOMENT_PARTS;
  const int nblk = (int)cdiv(trips, per);          // <= LTU_INTENSITY_MOMENT_PARTS, a function of n_voxels alone
  hipLaunchKernelGGL(intensity_moments_kernel, dim3(nblk), dim3(IM_THREADS), 0, st, img, lab, n_voxels, (unsigned)mask_bits, centre,
                     parts, per);
  hipLaunchKernelGGL(intensity_fold_kernel, dim3(1), dim3(64), 0, st, parts, nblk, out);
  return ltu_check_launch();
}
