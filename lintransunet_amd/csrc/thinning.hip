// Topology of binary volumes for the evaluation (no reference counterpart; tests/topology_common.py is the oracle): a
// topology-preserving curve skeleton by parallel thinning, the overlap counts of the clDice metric and the Euler characteristic.
// Integer work only: no floating-point atomics, two calls give the same bytes.
//
// Neighbourhood code of a voxel p: bit 9 (dh + 1) + 3 (dw + 1) + (dd + 1) is set when p + (dh, dw, dd) is object; voxels beyond the
// volume are background; bit 13 (the centre) is ignored.  N26 = all bits but 13, N18 = the bits with one or two nonzero offsets,
// N6 = the six face bits.
//   endpoint: exactly one bit of code & N26.
//   simple ((26, 6), Malandain-Bertrand): (a) code & N26 is non-empty and one component under 26-adjacency inside the 3x3x3 block,
//             (b) of the components of ~code & N18 under 6-adjacency restricted to N18, exactly one holds a bit of N6.
// th_flags evaluates both as bit-parallel flood fills in registers: a set of cells is a 27-bit word, a dilation is six masked shifts
// (the masks keep a bit on the far plane of an axis from wrapping into the next row), the box dilation of (a) is the three axes
// one after the other, the cross dilation of (b) their union.  (a) floods from the lowest object bit and compares with the whole
// set; (b) floods from the lowest background face bit and asks whether another face bit stayed outside.  At most 26 / 18 rounds,
// usually two or three; no table, no memory.
//
// Thinning (8-subfield sequential curve thinning with iteration-level border marking, Palagyi / Nemeth / Kardos): one iteration
//   1. mark: every object voxel with a background face neighbour in the image at the start of the iteration is a candidate;
//   2. for s = 0 .. 7: every candidate with (h & 1) | (w & 1) << 1 | (d & 1) << 2 == s forms its code from the CURRENT image and is
//      deleted when it is simple and not an endpoint.
// Two voxels of one subfield are never 26-adjacent, so a pass reads no voxel it writes: deleting at once and in place equals any
// sequential order, and the result does not depend on scheduling.  th_mark_kernel appends the candidates' linear indices (over all
// N volumes, < 2^32) to eight lists, one per subfield, with one integer atomic per wavefront and subfield after a ballot; list s
// starts at the sum of the object counts of the subfields before it (ltu_thin_count, read by the host once to size the lists) and
// cannot outgrow its share, since candidates are object voxels.  th_pass_kernel walks list s only, so an iteration costs one read
// of the volume (the mark) plus the surface.  A deletion is a byte store; neighbours are byte loads.  The order inside a list
// depends on scheduling; nothing that is stored does.
#include "common.h"

#define TH_HEADER 16                              // int32 elements before the lists: fill[8], the rest spare
#define TH_GRID 2048                              // workgroups of the grid-stride kernels
#define TH_MAX_ITERS 64

constexpr uint32_t th_plane(int axis, int value) {
  uint32_t m = 0;
  for (int i = 0; i < 27; ++i) {
    const int o[3] = {i / 9, (i / 3) % 3, i % 3};
    if (o[axis] == value) m |= 1u << i;
  }
  return m;
}
constexpr uint32_t th_ring(int lo, int hi) {       // the bits with lo .. hi nonzero offsets
  uint32_t m = 0;
  for (int i = 0; i < 27; ++i) {
    const int nz = (i / 9 != 1) + ((i / 3) % 3 != 1) + (i % 3 != 1);
    if (nz >= lo && nz <= hi) m |= 1u << i;
  }
  return m;
}
constexpr uint32_t TH_N26 = th_ring(1, 3), TH_N18 = th_ring(1, 2), TH_N6 = th_ring(1, 1);
constexpr uint32_t TH_A0 = th_plane(0, 0), TH_A2 = th_plane(0, 2), TH_B0 = th_plane(1, 0), TH_B2 = th_plane(1, 2),
                   TH_C0 = th_plane(2, 0), TH_C2 = th_plane(2, 2);
static_assert(TH_N26 == 0x7ffdfffu && __builtin_popcount(TH_N18) == 18 && __builtin_popcount(TH_N6) == 6, "neighbourhood masks");

__device__ __forceinline__ uint32_t th_dilate26(uint32_t x) {
  x |= ((x & ~TH_C2) << 1) | ((x & ~TH_C0) >> 1);
  x |= ((x & ~TH_B2) << 3) | ((x & ~TH_B0) >> 3);
  x |= ((x & ~TH_A2) << 9) | ((x & ~TH_A0) >> 9);
  return x;
}

__device__ __forceinline__ uint32_t th_dilate6(uint32_t x) {
  return x | ((x & ~TH_C2) << 1) | ((x & ~TH_C0) >> 1) | ((x & ~TH_B2) << 3) | ((x & ~TH_B0) >> 3) | ((x & ~TH_A2) << 9) |
         ((x & ~TH_A0) >> 9);
}

// bit 0 simple, bit 1 endpoint
__device__ __forceinline__ uint32_t th_flags(uint32_t code) {
  const uint32_t obj = code & TH_N26;
  const uint32_t endpoint = __builtin_popcount(obj) == 1 ? 2u : 0u;
  if (obj == 0) return 0;
  uint32_t r = obj & (0u - obj);
  for (int i = 0; i < 26; ++i) {
    const uint32_t n = th_dilate26(r) & obj;
    if (n == r) break;
    r = n;
  }
  if (r != obj) return endpoint;
  const uint32_t bg = ~code & TH_N18, faces = bg & TH_N6;
  if (faces == 0) return endpoint;
  r = faces & (0u - faces);
  for (int i = 0; i < 18; ++i) {
    const uint32_t n = th_dilate6(r) & bg;
    if (n == r) break;
    r = n;
  }
  return endpoint | ((faces & ~r) == 0 ? 1u : 0u);
}

__global__ void __launch_bounds__(256) th_codes_kernel(const uint32_t* __restrict__ codes, uint8_t* __restrict__ flags, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    flags[i] = (uint8_t)th_flags(codes[i]);
}

static bool th_shape_ok(int N, int H, int W, int D) {
  if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || D <= 0) return false;
  const long long S = (long long)H * W * D;
  return S < (1LL << 31) && S * N < (1LL << 32);
}

static unsigned th_grid(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > TH_GRID ? TH_GRID : b);
}

__device__ __forceinline__ int th_subfield(uint32_t h, uint32_t w, uint32_t d) { return (h & 1) | (w & 1) << 1 | (d & 1) << 2; }

// counts[s] += object voxels of subfield s over all volumes (zero before).  Uniform trip count: every lane reaches every ballot.
__global__ void __launch_bounds__(256) th_count_kernel(const uint8_t* __restrict__ vol, unsigned long long* __restrict__ counts,
                                                       unsigned long long total, uint32_t H, uint32_t W, uint32_t D) {
  unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < total; base += (unsigned long long)gridDim.x * 256) {
    const unsigned long long i = base + threadIdx.x;
    const bool obj = i < total && vol[i] != 0;
    if (__ballot(obj) == 0) continue;              // wave-uniform: most of a scan is background
    const uint32_t v = (uint32_t)i;
    const int sub = th_subfield((v / (W * D)) % H, (v / D) % W, v % D);
#pragma unroll
    for (int s = 0; s < 8; ++s) c[s] += __popcll(__ballot(obj && sub == s));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (c[s]) atomicAdd(&counts[s], c[s]);
  }
}

// appends every candidate to the list of its subfield.  list s starts at the sum of counts[0 .. s-1]; fill[s] (zero before) ends as
// its length.  A slot beyond the subfield's share or beyond cap is never written (counts that do not belong to vol lose
// candidates, they do not write out of bounds).
__global__ void __launch_bounds__(256) th_mark_kernel(const uint8_t* __restrict__ vol, const long long* __restrict__ counts,
                                                      uint32_t* __restrict__ list, int* __restrict__ fill, long long cap,
                                                      unsigned long long total, uint32_t H, uint32_t W, uint32_t D) {
  __shared__ long long off[8], share[8];
  if (threadIdx.x == 0) {
    long long a = 0;
    for (int s = 0; s < 8; ++s) {
      off[s] = a;
      share[s] = counts[s];
      a += counts[s];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const long long WD = (long long)W * D;
  for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < total; base += (unsigned long long)gridDim.x * 256) {
    const unsigned long long i = base + threadIdx.x;
    const bool obj = i < total && vol[i] != 0;
    if (__ballot(obj) == 0) continue;              // wave-uniform: most of a scan is background
    bool cand = false;
    int sub = 0;
    if (obj) {
      const uint32_t v = (uint32_t)i, d = v % D, w = (v / D) % W, h = (v / (W * D)) % H;
      const uint8_t* p = vol + i;
      cand = d == 0 || d == D - 1 || w == 0 || w == W - 1 || h == 0 || h == H - 1 || p[-1] == 0 || p[1] == 0 || p[-(long long)D] == 0 ||
             p[D] == 0 || p[-WD] == 0 || p[WD] == 0;
      sub = th_subfield(h, w, d);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool mine = cand && sub == s;
      const unsigned long long m = __ballot(mine);
      if (m == 0) continue;                        // wave-uniform
      const int leader = __ffsll((unsigned long long)m) - 1;
      int start = 0;
      if (lane == leader) start = atomicAdd(&fill[s], __popcll(m));
      start = __shfl(start, leader);
      if (mine) {
        const long long r = (long long)start + __popcll(m & below);
        if (r < share[s] && off[s] + r < cap) list[off[s] + r] = (uint32_t)i;
      }
    }
  }
}

// one subfield pass: the candidates of list s that are simple and not endpoints in the current image are cleared (byte stores);
// *deleted += their number
__global__ void __launch_bounds__(256) th_pass_kernel(uint8_t* __restrict__ vol, const long long* __restrict__ counts,
                                                      const uint32_t* __restrict__ list, const int* __restrict__ fill,
                                                      unsigned long long* __restrict__ deleted, long long cap, int s, int H, int W, int D) {
  long long off = 0;
  for (int t = 0; t < s; ++t) off += counts[t];
  long long n = fill[s];
  if (n > counts[s]) n = counts[s];
  if (n > cap - off) n = cap - off;
  const long long WD = (long long)W * D;
  int del = 0;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
    const uint32_t v = list[off + j];
    const int d = (int)(v % (uint32_t)D), w = (int)((v / (uint32_t)D) % (uint32_t)W), h = (int)((v / (uint32_t)(W * D)) % (uint32_t)H);
    uint8_t* p = vol + v;
    if (*p == 0) continue;
    uint32_t code = 0;
#pragma unroll
    for (int a = -1; a <= 1; ++a) {
      const bool ha = h + a >= 0 && h + a < H;
#pragma unroll
      for (int b = -1; b <= 1; ++b) {
        const bool wb = ha && w + b >= 0 && w + b < W;
#pragma unroll
        for (int c = -1; c <= 1; ++c) {
          if (a == 0 && b == 0 && c == 0) continue;
          if (wb && d + c >= 0 && d + c < D && p[a * WD + b * (long long)D + c] != 0) code |= 1u << (9 * (a + 1) + 3 * (b + 1) + (c + 1));
        }
      }
    }
    if (th_flags(code) == 1u) {
      *p = 0;
      ++del;
    }
  }
  for (int o = 32; o > 0; o >>= 1) del += __shfl_xor(del, o);
  if ((threadIdx.x & 63) == 0 && del) atomicAdd(deleted, (unsigned long long)del);
}

// ---- entry points: thinning -------------------------------------------------------------------------------------------------
extern "C" int ltu_thin_simple_codes(const uint32_t* codes, uint8_t* flags, long long n, ltu_stream_t s) {
  if (n <= 0 || n >= (1LL << 40)) return LTU_E_SHAPE;
  if (codes == nullptr || flags == nullptr) return LTU_E_ARG;
  hipLaunchKernelGGL(th_codes_kernel, dim3(th_grid(n)), dim3(256), 0, (hipStream_t)s, codes, flags, n);
  return ltu_check_launch();
}

extern "C" int ltu_thin_count(const uint8_t* vol, long long* counts, int N, int H, int W, int D, ltu_stream_t s) {
  if (!th_shape_ok(N, H, W, D)) return LTU_E_SHAPE;
  if (vol == nullptr || counts == nullptr) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long total = (long long)N * H * W * D;
  const hipError_t e = hipMemsetAsync(counts, 0, 8 * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(th_count_kernel, dim3(th_grid(total)), dim3(256), 0, st, vol, reinterpret_cast<unsigned long long*>(counts),
                     (unsigned long long)total, (uint32_t)H, (uint32_t)W, (uint32_t)D);
  return ltu_check_launch();
}

extern "C" long long ltu_thin_ws_elems(int N, int H, int W, int D, long long objects) {
  if (!th_shape_ok(N, H, W, D) || objects < 0 || objects > (long long)N * H * W * D) return 0;
  return TH_HEADER + objects;
}

extern "C" int ltu_thin_iterate(uint8_t* vol, const long long* counts, long long* deleted, int iters, int* scratch,
                                long long scratch_elems, long long objects, int N, int H, int W, int D, ltu_stream_t s) {
  if (!th_shape_ok(N, H, W, D) || iters < 1 || iters > TH_MAX_ITERS) return LTU_E_SHAPE;
  if (vol == nullptr || counts == nullptr || deleted == nullptr || objects < 0) return LTU_E_ARG;
  const long long need = ltu_thin_ws_elems(N, H, W, D, objects);
  if (scratch == nullptr || need == 0 || scratch_elems < need) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long total = (long long)N * H * W * D;
  int* fill = scratch;
  uint32_t* list = reinterpret_cast<uint32_t*>(scratch + TH_HEADER);
  hipError_t e = hipMemsetAsync(deleted, 0, (size_t)iters * sizeof(long long), st);
  const unsigned mark_grid = th_grid(total), pass_grid = th_grid(objects);
  for (int it = 0; it < iters && e == hipSuccess; ++it) {
    e = hipMemsetAsync(fill, 0, 8 * sizeof(int), st);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(th_mark_kernel, dim3(mark_grid), dim3(256), 0, st, vol, counts, list, fill, objects, (unsigned long long)total,
                       (uint32_t)H, (uint32_t)W, (uint32_t)D);
    for (int sub = 0; sub < 8; ++sub)
      hipLaunchKernelGGL(th_pass_kernel, dim3(pass_grid), dim3(256), 0, st, vol, counts, list, fill,
                         reinterpret_cast<unsigned long long*>(deleted) + it, objects, sub, H, W, D);
  }
  if (e != hipSuccess) return (int)e;
  return ltu_check_launch();
}

// ---- clDice: the two sides of every (sample, class) as volumes, and the overlap counts of their skeletons ---------------------
__device__ __forceinline__ int th_block_sum(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  const int sum = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return sum;
}

// out u8 [2][B][K][S]: side 0 = pred[b][k] >= thr, side 1 = target[b] == k, written at column kk.  grid = (blocks, B)
__global__ void __launch_bounds__(256) th_binarize_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ target,
                                                          uint8_t* __restrict__ out, int B, int C, int k, int kk, int K, long long S,
                                                          float thr) {
  const int b = blockIdx.y;
  const float* p = pred + ((long long)b * C + k) * S;
  const uint8_t* t = target + (long long)b * S;
  uint8_t* op = out + ((long long)b * K + kk) * S;
  uint8_t* og = op + (long long)B * K * S;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long long)gridDim.x * 256) {
    op[v] = p[v] >= thr;
    og[v] = t[v] == (uint8_t)k;
  }
}

// counts int32 [B][K][4] at column kk (zero before) += |S_P|, |S_P n G|, |S_G|, |S_G n P|.  grid = (blocks, B)
__global__ void __launch_bounds__(256) th_overlap_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ target,
                                                         const uint8_t* __restrict__ skel, int* __restrict__ counts, int B, int C, int k,
                                                         int kk, int K, long long S, float thr) {
  __shared__ int red[4];
  const int b = blockIdx.y;
  const float* p = pred + ((long long)b * C + k) * S;
  const uint8_t* t = target + (long long)b * S;
  const uint8_t* sp = skel + ((long long)b * K + kk) * S;
  const uint8_t* sg = sp + (long long)B * K * S;
  int c[4] = {0, 0, 0, 0};
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long long)gridDim.x * 256) {
    const bool inp = p[v] >= thr, ing = t[v] == (uint8_t)k, skp = sp[v] != 0, skg = sg[v] != 0;
    c[0] += skp;
    c[1] += skp && ing;
    c[2] += skg;
    c[3] += skg && inp;
  }
  for (int i = 0; i < 4; ++i) {
    const int sum = th_block_sum(c[i], red);
    if (threadIdx.x == 0 && sum) atomicAdd(&counts[((long long)b * K + kk) * 4 + i], sum);
  }
}

__global__ void th_overlap_zero_kernel(int* __restrict__ counts, int B, int K, int kk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 4 * B) counts[((long long)(i / 4) * K + kk) * 4 + (i % 4)] = 0;
}

// rates f32 [3][B][K] at column kk = clDice, Tprec, Tsens.  A non-empty set has a non-empty skeleton (thinning never deletes a
// component), so |S_X| = 0 says X is empty: both empty 1, one empty 0.
__global__ void th_rates_kernel(const int* __restrict__ counts, float* __restrict__ rates, int B, int K, int kk) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int* c = counts + ((long long)b * K + kk) * 4;
  double tprec, tsens, cl;
  if (c[0] == 0 && c[2] == 0) {
    tprec = tsens = cl = 1.0;
  } else if (c[0] == 0 || c[2] == 0) {
    tprec = tsens = cl = 0.0;
  } else {
    tprec = (double)c[1] / (double)c[0];
    tsens = (double)c[3] / (double)c[2];
    cl = tprec + tsens == 0.0 ? 0.0 : 2.0 * tprec * tsens / (tprec + tsens);
  }
  const long long at = (long long)b * K + kk, plane = (long long)B * K;
  rates[at] = (float)cl;
  rates[plane + at] = (float)tprec;
  rates[2 * plane + at] = (float)tsens;
}

static bool th_metric_shape_ok(int B, int C, int k, int kk, int K, int H, int W, int D) {
  return B > 0 && C > 0 && K > 0 && kk >= 0 && kk < K && k >= 0 && k < C && k < 256 && 2LL * B * K <= 65535 &&
         th_shape_ok(2 * B * K, H, W, D);
}

extern "C" int ltu_topology_binarize(const float* pred, const uint8_t* target, uint8_t* out, int B, int C, int k, int kk, int K, int H,
                                     int W, int D, float threshold, ltu_stream_t s) {
  if (!th_metric_shape_ok(B, C, k, kk, K, H, W, D)) return LTU_E_SHAPE;
  if (pred == nullptr || target == nullptr || out == nullptr || threshold != threshold) return LTU_E_ARG;
  const long long S = (long long)H * W * D;
  hipLaunchKernelGGL(th_binarize_kernel, dim3(th_grid(S), B), dim3(256), 0, (hipStream_t)s, pred, target, out, B, C, k, kk, K, S,
                     threshold);
  return ltu_check_launch();
}

extern "C" int ltu_topology_overlap(const float* pred, const uint8_t* target, const uint8_t* skel, int* counts, float* rates, int B,
                                    int C, int k, int kk, int K, int H, int W, int D, float threshold, ltu_stream_t s) {
  if (!th_metric_shape_ok(B, C, k, kk, K, H, W, D)) return LTU_E_SHAPE;
  if (pred == nullptr || target == nullptr || skel == nullptr || counts == nullptr || rates == nullptr || threshold != threshold)
    return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  hipLaunchKernelGGL(th_overlap_zero_kernel, dim3(cdiv(4 * B, 256)), dim3(256), 0, st, counts, B, K, kk);
  hipLaunchKernelGGL(th_overlap_kernel, dim3(th_grid(S), B), dim3(256), 0, st, pred, target, skel, counts, B, C, k, kk, K, S, threshold);
  hipLaunchKernelGGL(th_rates_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, counts, rates, B, K, kk);
  return ltu_check_launch();
}

// ---- Euler characteristic -----------------------------------------------------------------------------------------------------
// chi = V - E + F - C of the union of the closed unit cubes of the object voxels.  Lattice point q in [0, H] x [0, W] x [0, D] owns
// the vertex at q, the three edges and the three faces that start at q towards +h, +w, +d, and the cube of voxel q; each exists
// when one of the voxels around it is object, and all of those lie in the 2x2x2 block q - 1 .. q (beyond the volume: background).
// Integer partials, integer atomics: exact whatever the order.  grid = (blocks, N)
__global__ void __launch_bounds__(256) th_euler_kernel(const uint8_t* __restrict__ vol, unsigned long long* __restrict__ chi, int H, int W,
                                                       int D) {
  __shared__ int red[4];
  const uint8_t* vb = vol + (long long)blockIdx.y * ((long long)H * W * D);
  const long long W1 = W + 1, D1 = D + 1, Q = (long long)(H + 1) * W1 * D1;
  int sum = 0;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < Q; q += (long long)gridDim.x * 256) {
    const int d = (int)(q % D1), w = (int)((q / D1) % W1), h = (int)(q / (D1 * W1));
    bool v[2][2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int hh = h - 1 + a, ww = w - 1 + b, dd = d - 1 + c;
          v[a][b][c] = hh >= 0 && hh < H && ww >= 0 && ww < W && dd >= 0 && dd < D && vb[((long long)hh * W + ww) * D + dd] != 0;
        }
    const bool cube = v[1][1][1];
    const bool fh = cube || v[0][1][1], fw = cube || v[1][0][1], fd = cube || v[1][1][0];      // the faces across h, w, d
    const bool eh = fw || v[1][1][0] || v[1][0][0], ew = fh || v[1][1][0] || v[0][1][0], ed = fh || v[1][0][1] || v[0][0][1];
    const bool vert = eh || v[0][1][1] || v[0][1][0] || v[0][0][1] || v[0][0][0];
    sum += (int)vert - ((int)eh + (int)ew + (int)ed) + ((int)fh + (int)fw + (int)fd) - (int)cube;
  }
  sum = th_block_sum(sum, red);
  if (threadIdx.x == 0 && sum) atomicAdd(&chi[blockIdx.y], (unsigned long long)(long long)sum);
}

extern "C" int ltu_euler_characteristic(const uint8_t* vol, long long* chi, int N, int H, int W, int D, ltu_stream_t s) {
  if (!th_shape_ok(N, H, W, D)) return LTU_E_SHAPE;
  if (vol == nullptr || chi == nullptr) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const hipError_t e = hipMemsetAsync(chi, 0, (size_t)N * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  const long long Q = (long long)(H + 1) * (W + 1) * (D + 1);
  hipLaunchKernelGGL(th_euler_kernel, dim3(th_grid(Q), N), dim3(256), 0, st, vol, reinterpret_cast<unsigned long long*>(chi), H, W, D);
  return ltu_check_launch();
}
