// Crop index of one scan's label (data side; no reference counterpart: monai's RandCropByPosNegLabeld / RandCropByLabelClassesd
// keep np.nonzero index lists on the host, O(voxels) per list).  The u8 label [H][W][D] (n voxels in raster order) is cut into
// blocks of CI_BLOCK voxels; every voxel falls into one of 9 bins: its value 0 .. 7, or bin 8 for every value >= 8.
//   build:  crop_index_count_kernel   one wave per block counts its voxels per bin                 -> index[bin][block]
//           crop_index_scan_kernel    one workgroup per bin turns the counts into exclusive prefixes in place, index[bin][nb] =
//                                     the bin's population, also written to totals[bin] (u64)
//   select: crop_index_select_kernel  one wave per query (mask, rank): the set is the union of the bins whose bit is set in mask
//                                     (bit 0 background, bits 1 .. 8 foreground); the prefix of a union is the sum of its bins'
//                                     prefixes, so a 64-way search over the blocks finds the one block that holds the rank-th member,
//                                     and that block alone is read: lane l owns the 64-byte strip l of it, marks its members in a
//                                     64-bit word, a wave prefix of the popcounts finds the lane and the rank inside the strip the bit.
// Index layout: uint32 [9][nb + 1], nb = ceil(n / CI_BLOCK).  n <= 2^32 - 1, so every prefix and population fits 32 bits.
// Integer arithmetic only, no atomics, every element of the index is written by every build: two builds are byte-identical.
// Voxels at or beyond n are neither loaded nor counted (a 16-byte chunk that straddles n is read byte by byte below n).
#include "common.h"

#define CI_BLOCK 4096                              // voxels per block: a 64-byte strip per lane of one wave
#define CI_BINS 9
#define CI_MAX_VOXELS 0xffffffffLL

static bool ci_size_ok(long long n) { return n >= 1 && n <= CI_MAX_VOXELS; }
static long long ci_nblocks(long long n) { return (n + CI_BLOCK - 1) / CI_BLOCK; }

__device__ __forceinline__ unsigned ci_bin(unsigned v) { return v < 8u ? v : 8u; }

// the bytes [off, off + 16) of lab that lie below n, as four little-endian words (zero where nothing was loaded); returns how
// many of the 16 are valid.  lab is 16-byte aligned and off a multiple of 16.
__device__ __forceinline__ int ci_load16(const uint8_t* __restrict__ lab, long long off, long long n, uint32_t w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0u;
  if (off + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(lab + off);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    return 16;
  }
  if (off >= n) return 0;
  const int valid = (int)(n - off);
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < valid) w[k >> 2] |= (uint32_t)lab[off + k] << (8 * (k & 3));
  return valid;
}

// one wave per block, four blocks per workgroup.  Chunk j of lane l is bytes (j * 64 + l) * 16 of the block: the order inside a
// block does not matter for a count, so the loads are the coalesced ones.  A lane sees at most 64 voxels: nine 7-bit counters in
// one 64-bit word.
__global__ void __launch_bounds__(256) crop_index_count_kernel(const uint8_t* __restrict__ lab, long long n, uint32_t* __restrict__ index,
                                                               int nb) {
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nb) return;                           // wave-uniform
  const long long base = (long long)blk * CI_BLOCK;
  unsigned long long acc = 0ull;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t w[4];
    const int valid = ci_load16(lab, base + (long long)(j * 64 + lane) * 16, n, w);
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < valid) acc += 1ull << (7 * ci_bin((w[k >> 2] >> (8 * (k & 3))) & 0xffu));
  }
#pragma unroll
  for (int b = 0; b < CI_BINS; ++b) {
    unsigned c = (unsigned)(acc >> (7 * b)) & 0x7fu;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) index[(long long)b * (nb + 1) + blk] = c;
  }
}

// workgroup b: index[b][0 .. nb) from counts to exclusive prefixes in place (a thread reads and writes its own run of blocks only),
// index[b][nb] = totals[b] = the population of bin b
#define CI_SCAN_THREADS 1024
__global__ void __launch_bounds__(CI_SCAN_THREADS) crop_index_scan_kernel(uint32_t* __restrict__ index,
                                                                          unsigned long long* __restrict__ totals, int nb) {
  constexpr int NW = CI_SCAN_THREADS / 64;
  __shared__ unsigned red[NW];
  __shared__ unsigned wpre[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* c = index + (long long)blockIdx.x * (nb + 1);
  const int per = (nb + CI_SCAN_THREADS - 1) / CI_SCAN_THREADS;
  const int i0 = min(tid * per, nb), i1 = min(i0 + per, nb);
  unsigned s = 0u;
  for (int i = i0; i < i1; ++i) s += c[i];
  unsigned inc = s;                                // inclusive scan over the wave, then over the waves
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned u = __shfl_up(inc, d);
    if (lane >= d) inc += u;
  }
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  if (tid == 0) {
    unsigned a = 0u;
    for (int w = 0; w < NW; ++w) { wpre[w] = a; a += red[w]; }
    c[nb] = a;
    totals[blockIdx.x] = a;
  }
  __syncthreads();
  unsigned run = wpre[wave] + inc - s;
  for (int i = i0; i < i1; ++i) {
    const unsigned v = c[i];
    c[i] = run;
    run += v;
  }
}

// members of the set before block b (b = nb: the set's population)
__device__ __forceinline__ unsigned long long ci_prefix(const uint32_t* __restrict__ index, int nb, unsigned mask, int b) {
  unsigned long long p = 0ull;
#pragma unroll
  for (int k = 0; k < CI_BINS; ++k)
    if ((mask >> k) & 1u) p += index[(long long)k * (nb + 1) + b];
  return p;
}

// one wave per query, four queries per workgroup
__global__ void __launch_bounds__(256) crop_index_select_kernel(const uint8_t* __restrict__ lab, long long n,
                                                                const uint32_t* __restrict__ index, int nb,
                                                                const uint32_t* __restrict__ queries, long long* __restrict__ out, int nq) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;                             // wave-uniform
  const unsigned mask = queries[2 * q] & 0x1ffu;
  const unsigned long long rank = queries[2 * q + 1];
  if (rank >= ci_prefix(index, nb, mask, nb)) {    // also the empty mask
    if (lane == 0) out[q] = -1;
    return;
  }
  // prefix(lo) <= rank < prefix(hi), both wave-uniform.  A 64-way step: lane l probes block lo + (l + 1) * step; the prefixes do
  // not decrease, so the probes at or below rank are the first k lanes, and the member lies in [lo + k * step, lo + (k + 1) * step).
  // Three dependent rounds of loads for up to 2^18 blocks, four beyond, where a binary search takes one per bit.
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) / 64;
    const int p = lo + (lane + 1) * step;
    const int k = __popcll(__ballot(p < hi && ci_prefix(index, nb, mask, p) <= rank));
    lo += k * step;
    hi = min(lo + step, hi);
  }
  const unsigned r = (unsigned)(rank - ci_prefix(index, nb, mask, lo));      // < CI_BLOCK for an index built from this label
  const long long base = (long long)lo * CI_BLOCK + lane * 64;
  unsigned long long member = 0ull;                // bit i: byte i of this lane's strip is in the set
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t w[4];
    const int valid = ci_load16(lab, base + j * 16, n, w);
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < valid && ((mask >> ci_bin((w[k >> 2] >> (8 * (k & 3))) & 0xffu)) & 1u)) member |= 1ull << (j * 16 + k);
  }
  const unsigned cnt = (unsigned)__popcll(member);
  unsigned inc = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned u = __shfl_up(inc, d);
    if (lane >= d) inc += u;
  }
  const unsigned exc = inc - cnt;
  const bool mine = exc <= r && r < inc;
  if (mine) {
    for (unsigned k = r - exc; k > 0; --k) member &= member - 1;      // drop the members before it
    out[q] = base + (__ffsll(member) - 1);
  }
  if (__ballot(mine) == 0ull && lane == 0) out[q] = -1;                // the label changed after the build: no value
}

extern "C" long long ltu_crop_index_elems(long long n_voxels) {
  if (!ci_size_ok(n_voxels)) return 0;
  return CI_BINS * (ci_nblocks(n_voxels) + 1);
}

static int ci_check(const uint8_t* lab, long long n_voxels, const uint32_t* index, long long index_elems) {
  if (!ci_size_ok(n_voxels)) return LTU_E_SHAPE;
  if (lab == nullptr || index == nullptr || index_elems < ltu_crop_index_elems(n_voxels)) return LTU_E_ARG;
  if (((uintptr_t)lab & 15) != 0 || ((uintptr_t)index & 3) != 0) return LTU_E_ALIGN;
  return LTU_OK;
}

extern "C" int ltu_crop_index_build(const uint8_t* lab, long long n_voxels, uint32_t* index, long long index_elems,
                                    unsigned long long* totals, ltu_stream_t s) {
  const int rc = ci_check(lab, n_voxels, index, index_elems);
  if (rc != LTU_OK) return rc;
  if (totals == nullptr) return LTU_E_ARG;
  if (((uintptr_t)totals & 7) != 0) return LTU_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  const int nb = (int)ci_nblocks(n_voxels);
  hipLaunchKernelGGL(crop_index_count_kernel, dim3(cdiv(nb, 4)), dim3(256), 0, st, lab, n_voxels, index, nb);
  hipLaunchKernelGGL(crop_index_scan_kernel, dim3(CI_BINS), dim3(CI_SCAN_THREADS), 0, st, index, totals, nb);
  return ltu_check_launch();
}

extern "C" int ltu_crop_index_select(const uint8_t* lab, long long n_voxels, const uint32_t* index, long long index_elems,
                                     const uint32_t* queries, long long* out, int n, ltu_stream_t s) {
  const int rc = ci_check(lab, n_voxels, index, index_elems);
  if (rc != LTU_OK) return rc;
  if (n < 0 || (n > 0 && (queries == nullptr || out == nullptr))) return LTU_E_ARG;
  if (n == 0) return LTU_OK;
  if (((uintptr_t)queries & 3) != 0 || ((uintptr_t)out & 7) != 0) return LTU_E_ALIGN;
  const int nb = (int)ci_nblocks(n_voxels);
  hipLaunchKernelGGL(crop_index_select_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)s, lab, n_voxels, index, nb, queries, out, n);
  return ltu_check_launch();
}
