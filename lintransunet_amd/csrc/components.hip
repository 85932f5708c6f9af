// Connected-component labelling, small-component removal and lesion-wise detection metrics of the evaluation (no reference
// counterpart; scipy.ndimage.label is the oracle).  Connectivity c = 1, 2, 3: two voxels are adjacent when their coordinates
// differ by at most 1 on every axis and on at most c axes (6, 18, 26 neighbours); voxels beyond the volume are background.
//
// Labelling is a union-find over voxel indices of one sample (S = H W D < 2^31) in a fixed number of launches, no host loop:
//   1. cc_local_kernel: one 8x16x32 tile per workgroup is labelled in LDS (every fg voxel its own parent, union with the 3 / 9 /
//      13 neighbours of the half-neighbourhood already visited, atomicMin keeps the smaller index as root, full compression);
//      par[v] = the global index of its tile-local root, -1 for background.
//   2. cc_merge_kernel: the voxels on tile faces union across faces in global memory (global atomics ~ tile faces, not voxels).
//   3. cc_compress_kernel: par[v] = find(v) for every fg voxel (full path compression); roots counted per block of 4096.
//   4. cc_scan_kernel: per-sample exclusive scan of the block counts (one workgroup per sample), counts[b] = n_b.
//   5. cc_rank_kernel: each root, in raster order, stores -(rank + 2) in its own par slot.
//   6. cc_fill_kernel: labels[v] = rank(root(v)) + 1, 0 for background.
// Union by atomicMin makes the root of every set its smallest voxel index, the raster-first voxel of the component, so ranking the
// roots in index order reproduces scipy's numbering, whatever the scheduling.  Cross-workgroup visibility: a plain load may return
// a stale (older, larger) parent from another XCD's L2; parents only ever decrease and every older parent is still an ancestor, so
// a stale read costs iterations only: every union decision is taken from the value atomicMin returns.  Phases are kernels.
//
// Small-component removal: labelling steps 1-3, then a root-indexed histogram (equal roots aggregated along the wave before the
// atomic: runs along D are the common case) and a clearing pass; channel 0 = 1 - the rest at the end.
//
// Largest component (inference_multi_classes.py:104,148-151): the same labelling and histogram on the union of the foreground
// channels, then per sample an atomicMax of (size << 32) | (0xFFFFFFFF - root) over the roots: integer atomics, so the order does
// not matter, and among equally large components the smaller root = the raster-first one wins, as bincount / argmax decide it.
// A clearing pass zeroes channels 1 .. C-1 of every other component; channel 0 = 1 - the rest at the end.
//
// Hole filling (scipy.ndimage.binary_fill_holes; monai FillHoles): labelling steps 1-3 of the mask's COMPLEMENT, one pass over the
// six faces of the volume stores a mark in the root slot of every background component that reaches a face (every writer stores
// the same value: plain stores), one pass writes mask u {background whose root carries no mark}.  Five launches, no host read.
//
// Lesion statistics per (sample, class): P and G labelled (steps 1-3) into two parent arrays; one pass histograms |P_i|, |G_j|,
// |P_i n G|, |G_j n P| by root; one pass inserts the distinct (root P, root G) pairs into a per-sample hash set of 64-bit keys
// (atomicCAS, linear probing) from the "heads" of P n G only (voxels of P n G without a half-neighbour in P n G: every connected
// piece of P n G has one, and a piece lies inside one pair) and adds |P_i| into U_j for each new pair; per-block partials (Dice_j
// in fp64 in a fixed order, integer counts) are folded in a fixed order by one workgroup per sample.  All counts are integers:
// two calls are bit-identical.
#include "common.h"

#define CC_TH 8
#define CC_TW 16
#define CC_TD 32
#define CC_TILE (CC_TH * CC_TW * CC_TD)          // 4096 voxels, 16 per lane
#define CC_RB 4096                                // voxels per block of the root count / rank / partial passes
#define CC_EMPTY 0xffffffffffffffffull

// a binary source plane: kind 0 u8 != 0, 1 f32 >= thr, 2 f32 > thr, 3 u8 == cls, 4 the f32 sum of channels 1 .. cls - 1 (planes
// `plane` elements apart, added in channel order) > 0, 5 u8 == 0 (the complement of a mask); sample b starts at p + b * stride
// elements
struct cc_src {
  const void* p;
  long long stride;
  int kind;
  int cls;
  float thr;
  long long plane;
};

__device__ __forceinline__ bool cc_fg(const cc_src& s, int b, long long i) {
  const long long o = (long long)b * s.stride + i;
  switch (s.kind) {
    case 0: return static_cast<const uint8_t*>(s.p)[o] != 0;
    case 1: return static_cast<const float*>(s.p)[o] >= s.thr;
    case 2: return static_cast<const float*>(s.p)[o] > s.thr;
    case 3: return static_cast<const uint8_t*>(s.p)[o] == (uint8_t)s.cls;
    case 5: return static_cast<const uint8_t*>(s.p)[o] == 0;
    default: {
      float fg = 0.f;
      for (int c = 1; c < s.cls; ++c) fg += static_cast<const float*>(s.p)[o + c * s.plane];
      return fg > 0.f;
    }
  }
}

// the half-neighbourhood already visited in raster order: the first 3 (c = 1), 9 (c = 2) or 13 (c = 3) offsets (dh, dw, dd)
__constant__ int8_t cc_off[13][3] = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1},
                                     {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},
                                     {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

static bool cc_shape_ok(int B, int H, int W, int D) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && D > 0 && (long long)H * W * D < (1LL << 31);
}

static long long cc_nblocks(int H, int W, int D) { return ((long long)H * W * D + CC_RB - 1) / CC_RB; }

// ---- union-find in LDS (one workgroup) -------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_lfind(int* lp, int x) {
  while (true) {
    const int q = __hip_atomic_load(&lp[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (q == x) return x;
    x = q;
  }
}

__device__ __forceinline__ void cc_lunion(int* lp, int a, int b) {
  while (true) {
    a = cc_lfind(lp, a);
    b = cc_lfind(lp, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lp[b], a);        // link the larger root under the smaller one
    if (old == b) return;
    b = old;                                     // b had been linked meanwhile: merge its (former) parent instead
  }
}

// ---- union-find in global memory ------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_gfind(int* par, int x) {
  while (true) {
    const int q = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == x) return x;
    x = q;                                        // stale q is an older ancestor: still on the path to the root
  }
}

__device__ __forceinline__ void cc_gunion(int* par, int a, int b) {
  while (true) {
    a = cc_gfind(par, a);
    b = cc_gfind(par, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[b], a);        // the decision comes from the atomic's return, never from a plain load
    if (old == b) return;
    b = old;
  }
}

// 1. tile-local labelling.  grid = (tiles, B); par of sample b at par + b * S.
template <int NOFF>
__global__ void __launch_bounds__(256) cc_local_kernel(cc_src src, int* __restrict__ par, int H, int W, int D, int ntw, int ntd) {
  __shared__ int lp[CC_TILE];
  const int b = blockIdx.y, t = blockIdx.x;
  const int td = t % ntd, tw = (t / ntd) % ntw, th = t / (ntd * ntw);
  const int h0 = th * CC_TH, w0 = tw * CC_TW, d0 = td * CC_TD;
  const long long S = (long long)H * W * D;
  int* pb = par + (long long)b * S;
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    const int lh = i / (CC_TW * CC_TD), lw = (i / CC_TD) % CC_TW, ld = i % CC_TD;
    const int h = h0 + lh, w = w0 + lw, d = d0 + ld;
    const bool in = h < H && w < W && d < D;
    lp[i] = in && cc_fg(src, b, ((long long)h * W + w) * D + d) ? i : -1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    if (lp[i] < 0) continue;                      // fg-ness never changes: lp[i] >= 0 stays >= 0
    const int lh = i / (CC_TW * CC_TD), lw = (i / CC_TD) % CC_TW, ld = i % CC_TD;
#pragma unroll
    for (int o = 0; o < NOFF; ++o) {
      const int nh = lh + cc_off[o][0], nw = lw + cc_off[o][1], nd = ld + cc_off[o][2];
      if (nh < 0 || nw < 0 || nd < 0 || nw >= CC_TW || nd >= CC_TD) continue;     // other tile (or beyond the volume)
      const int n = (nh * CC_TW + nw) * CC_TD + nd;
      if (lp[n] >= 0) cc_lunion(lp, i, n);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    const int lh = i / (CC_TW * CC_TD), lw = (i / CC_TD) % CC_TW, ld = i % CC_TD;
    const int h = h0 + lh, w = w0 + lw, d = d0 + ld;
    if (h >= H || w >= W || d >= D) continue;
    int g = -1;
    if (lp[i] >= 0) {
      const int r = cc_lfind(lp, i);
      const int rh = r / (CC_TW * CC_TD), rw = (r / CC_TD) % CC_TW, rd = r % CC_TD;
      g = (int)(((long long)(h0 + rh) * W + (w0 + rw)) * D + (d0 + rd));
    }
    pb[((long long)h * W + w) * D + d] = g;
  }
}

// 2. unions across tile faces: a fg voxel on a face of its tile unions with each fg half-neighbour in another tile
template <int NOFF>
__global__ void __launch_bounds__(256) cc_merge_kernel(int* __restrict__ par, int H, int W, int D, int ntw, int ntd) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int td = t % ntd, tw = (t / ntd) % ntw, th = t / (ntd * ntw);
  const int h0 = th * CC_TH, w0 = tw * CC_TW, d0 = td * CC_TD;
  const long long S = (long long)H * W * D;
  int* pb = par + (long long)b * S;
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    const int lh = i / (CC_TW * CC_TD), lw = (i / CC_TD) % CC_TW, ld = i % CC_TD;
    if (lh != 0 && lw != 0 && ld != 0 && lw != CC_TW - 1 && ld != CC_TD - 1) continue;      // interior: merged in LDS
    const int h = h0 + lh, w = w0 + lw, d = d0 + ld;
    if (h >= H || w >= W || d >= D) continue;
    const int v = (int)(((long long)h * W + w) * D + d);
    if (pb[v] < 0) continue;
#pragma unroll
    for (int o = 0; o < NOFF; ++o) {
      const int lnh = lh + cc_off[o][0], lnw = lw + cc_off[o][1], lnd = ld + cc_off[o][2];
      if (lnh >= 0 && lnw >= 0 && lnd >= 0 && lnw < CC_TW && lnd < CC_TD) continue;     // same tile
      const int nh = h + cc_off[o][0], nw = w + cc_off[o][1], nd = d + cc_off[o][2];
      if (nh < 0 || nw < 0 || nd < 0 || nw >= W || nd >= D) continue;
      const int n = (int)(((long long)nh * W + nw) * D + nd);
      if (pb[n] >= 0) cc_gunion(pb, v, n);
    }
  }
}

__device__ __forceinline__ int cc_block_sum(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  const int s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

// 3. full path compression and roots per block.  grid = (nb, B); cnt [B][nb] (nullable)
__global__ void __launch_bounds__(256) cc_compress_kernel(int* __restrict__ par, int* __restrict__ cnt, long long S, int nb) {
  __shared__ int red[4];
  const int b = blockIdx.y;
  int* pb = par + (long long)b * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  int roots = 0;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    const int p = pb[v];
    if (p < 0) continue;
    const int r = cc_gfind(pb, p);
    if (r != p) __hip_atomic_store(&pb[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    roots += r == (int)v;
  }
  roots = cc_block_sum(roots, red);
  if (cnt != nullptr && threadIdx.x == 0) cnt[(long long)b * nb + blockIdx.x] = roots;
}

// 4. exclusive scan of the block counts of one sample per workgroup; counts[b] = number of components
__global__ void __launch_bounds__(256) cc_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off, int* __restrict__ counts,
                                                      int nb) {
  __shared__ int red[4];
  __shared__ int wpre[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* c = cnt + (long long)b * nb;
  int* o = off + (long long)b * nb;
  const int per = (nb + 255) / 256, i0 = tid * per, i1 = min(i0 + per, nb);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += c[i];
  int inc = s;                                    // inclusive scan over the wave, then over the four waves
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d);
    if (lane >= d) inc += u;
  }
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  if (tid == 0) {
    int a = 0;
    for (int w = 0; w < 4; ++w) { wpre[w] = a; a += red[w]; }
    counts[b] = a;
  }
  __syncthreads();
  int run = wpre[wave] + inc - s;
  for (int i = i0; i < i1; ++i) { o[i] = run; run += c[i]; }
}

// 5. each root stores -(rank + 2) in its own slot, rank = its position among the sample's roots in raster order
__global__ void __launch_bounds__(256) cc_rank_kernel(int* __restrict__ par, const int* __restrict__ off, long long S, int nb) {
  __shared__ int wcnt[2][4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int* pb = par + (long long)b * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  int run = off[(long long)b * nb + blockIdx.x];
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int j = 0; j < CC_RB / 256; ++j) {         // uniform trip count: every lane reaches every barrier
    const long long v = base + j * 256 + threadIdx.x;
    const bool root = v < S && pb[v] == (int)v;
    const unsigned long long m = __ballot(root);
    if (lane == 0) wcnt[j & 1][wave] = __popcll(m);
    __syncthreads();
    int pre = run, tot = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) pre += wcnt[j & 1][w];
      tot += wcnt[j & 1][w];
    }
    if (root) pb[v] = -(pre + __popcll(m & below) + 2);
    run += tot;
  }
}

// 6. labels from the ranks: -1 background, <= -2 a root's own rank, >= 0 the root (after compression).  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_fill_kernel(const int* __restrict__ par, int* __restrict__ labels, long long S) {
  const int* pb = par + (long long)blockIdx.y * S;
  int* lb = labels + (long long)blockIdx.y * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    const int p = pb[v];
    lb[v] = p == -1 ? 0 : p <= -2 ? -p - 1 : -pb[p] - 1;
  }
}

static void cc_grid(int H, int W, int D, int* ntw, int* ntd, int* ntiles) {
  const int nth = (H + CC_TH - 1) / CC_TH;
  *ntw = (W + CC_TW - 1) / CC_TW;
  *ntd = (D + CC_TD - 1) / CC_TD;
  *ntiles = nth * *ntw * *ntd;
}

// steps 1-3: par [B][S] = the root (smallest index) of every fg voxel's component, -1 for background; cnt [B][nb] roots per block
static void cc_label_roots(const cc_src& src, int* par, int* cnt, int B, int H, int W, int D, int connectivity, hipStream_t st) {
  int ntw, ntd, ntiles;
  cc_grid(H, W, D, &ntw, &ntd, &ntiles);
  const dim3 tg((unsigned)ntiles, B);
  switch (connectivity) {
    case 1:
      hipLaunchKernelGGL(cc_local_kernel<3>, tg, dim3(256), 0, st, src, par, H, W, D, ntw, ntd);
      hipLaunchKernelGGL(cc_merge_kernel<3>, tg, dim3(256), 0, st, par, H, W, D, ntw, ntd);
      break;
    case 2:
      hipLaunchKernelGGL(cc_local_kernel<9>, tg, dim3(256), 0, st, src, par, H, W, D, ntw, ntd);
      hipLaunchKernelGGL(cc_merge_kernel<9>, tg, dim3(256), 0, st, par, H, W, D, ntw, ntd);
      break;
    default:
      hipLaunchKernelGGL(cc_local_kernel<13>, tg, dim3(256), 0, st, src, par, H, W, D, ntw, ntd);
      hipLaunchKernelGGL(cc_merge_kernel<13>, tg, dim3(256), 0, st, par, H, W, D, ntw, ntd);
      break;
  }
  const long long S = (long long)H * W * D;
  const int nb = (int)cc_nblocks(H, W, D);
  hipLaunchKernelGGL(cc_compress_kernel, dim3(nb, B), dim3(256), 0, st, par, cnt, S, nb);
}

// ---- labelling entry points ----------------------------------------------------------------------------------------------
extern "C" long long ltu_label_ws_elems(int B, int H, int W, int D) {
  if (!cc_shape_ok(B, H, W, D)) return 0;
  return (long long)B * ((long long)H * W * D + 2 * cc_nblocks(H, W, D));
}

extern "C" int ltu_label_components(const uint8_t* mask, int* labels, int* counts, int* scratch, long long scratch_elems, int B,
                                    int H, int W, int D, int connectivity, ltu_stream_t s) {
  if (!cc_shape_ok(B, H, W, D)) return LTU_E_SHAPE;
  if (connectivity < 1 || connectivity > 3) return LTU_E_ARG;
  if (mask == nullptr || labels == nullptr || counts == nullptr) return LTU_E_ARG;
  if (scratch == nullptr || scratch_elems < ltu_label_ws_elems(B, H, W, D)) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  const int nb = (int)cc_nblocks(H, W, D);
  int* par = scratch;
  int* cnt = par + (long long)B * S;
  int* off = cnt + (long long)B * nb;
  const cc_src src{mask, S, 0, 0, 0.f};
  cc_label_roots(src, par, cnt, B, H, W, D, connectivity, st);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(B), dim3(256), 0, st, cnt, off, counts, nb);
  hipLaunchKernelGGL(cc_rank_kernel, dim3(nb, B), dim3(256), 0, st, par, off, S, nb);
  hipLaunchKernelGGL(cc_fill_kernel, dim3(nb, B), dim3(256), 0, st, par, labels, S);
  return ltu_check_launch();
}


// ---- small-component removal ---------------------------------------------------------------------------------------------
// arr[key] += the length of the run of equal keys this lane starts (key < 0: nothing).  Every lane of the wave calls it: one
// atomic per run instead of one per voxel (Guideline 12; lanes run along D, where runs are the common case).
__device__ __forceinline__ void cc_wave_hist(int* arr, int key) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const unsigned long long heads = __ballot(head);
  if (head && key >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run = above ? __ffsll((unsigned long long)above) : 64 - lane;
    atomicAdd(&arr[key], run);
  }
}

// size[b][root] = voxels of the component.  grid = (nb, B); uniform trip count (every lane reaches every ballot)
__global__ void __launch_bounds__(256) cc_size_kernel(const int* __restrict__ par, int* __restrict__ size, long long S) {
  const int* pb = par + (long long)blockIdx.y * S;
  int* sb = size + (long long)blockIdx.y * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    cc_wave_hist(sb, v < S ? pb[v] : -1);
  }
}

// channel k of sample b cleared where its component has fewer than min_voxels voxels.  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_clear_kernel(float* __restrict__ pred, const int* __restrict__ par, const int* __restrict__ size,
                                                       long long S, int C, int k, int min_voxels) {
  const int b = blockIdx.y;
  const int* pb = par + (long long)b * S;
  const int* sb = size + (long long)b * S;
  float* out = pred + ((long long)b * C + k) * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    const int p = pb[v];
    if (p >= 0 && sb[p] < min_voxels) out[v] = 0.f;
  }
}

// channel 0 = 1 - the sum of the other channels.  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_channel0_kernel(float* __restrict__ pred, long long S, int C) {
  float* p = pred + (long long)blockIdx.y * C * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    float sum = 0.f;
    for (int c = 1; c < C; ++c) sum += p[c * S + v];
    p[v] = 1.f - sum;
  }
}

// best[b] = the largest (size << 32) | (0xFFFFFFFF - root) over the non-empty roots of sample b (zero before).  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_pick_kernel(const int* __restrict__ size, unsigned long long* __restrict__ best, long long S) {
  const int* sb = size + (long long)blockIdx.y * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    const int n = sb[v];
    if (n > 0) atomicMax(&best[blockIdx.y], ((unsigned long long)(unsigned)n << 32) | (0xFFFFFFFFu - (unsigned)v));
  }
}

// channels 1 .. C-1 of sample b cleared at the fg voxels whose root is not the one in best[b].  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_keep_kernel(float* __restrict__ pred, const int* __restrict__ par,
                                                      const unsigned long long* __restrict__ best, long long S, int C) {
  const int b = blockIdx.y;
  const int* pb = par + (long long)b * S;
  float* out = pred + (long long)b * C * S;
  const int keep = (int)(0xFFFFFFFFu - (unsigned)(best[b] & 0xFFFFFFFFull));
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    const int p = pb[v];
    if (p < 0 || p == keep) continue;
    for (int c = 1; c < C; ++c) out[c * S + v] = 0.f;
  }
}

// what the in-place entry points refuse before any launch; need = their scratch query
static int cc_inplace_check(const float* pred, const int* scratch, long long scratch_elems, long long need, int B, int C, int H, int W,
                            int D, int connectivity) {
  if (!cc_shape_ok(B, H, W, D) || C < 2 || C > 31) return LTU_E_SHAPE;
  if (connectivity < 1 || connectivity > 3 || pred == nullptr || scratch == nullptr || scratch_elems < need) return LTU_E_ARG;
  return LTU_OK;
}

// labelling steps 1-3 of src into par = scratch [B][S], then size = scratch + B S [B][S] = voxels per root; the `zeroed` elements
// from size on are cleared first (size itself, and what the caller keeps behind it)
static int cc_label_sizes(const cc_src& src, int* scratch, long long zeroed, int B, int H, int W, int D, int connectivity,
                          hipStream_t st) {
  const long long S = (long long)H * W * D;
  int* size = scratch + (long long)B * S;
  cc_label_roots(src, scratch, nullptr, B, H, W, D, connectivity, st);
  const hipError_t e = hipMemsetAsync(size, 0, (size_t)zeroed * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(cc_size_kernel, dim3((unsigned)cc_nblocks(H, W, D), B), dim3(256), 0, st, scratch, size, S);
  return LTU_OK;
}

extern "C" long long ltu_remove_small_ws_elems(int B, int H, int W, int D) {
  if (!cc_shape_ok(B, H, W, D)) return 0;
  return (long long)B * 2 * ((long long)H * W * D);
}

extern "C" int ltu_remove_small_components(float* pred, int* scratch, long long scratch_elems, int B, int C, int classes, int H, int W,
                                           int D, int min_voxels, int connectivity, ltu_stream_t s) {
  const int refused = cc_inplace_check(pred, scratch, scratch_elems, ltu_remove_small_ws_elems(B, H, W, D), B, C, H, W, D, connectivity);
  if (refused != LTU_OK) return refused;
  if ((classes & 1) || (classes >> C) != 0) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  const int nb = (int)cc_nblocks(H, W, D);
  int* par = scratch;
  int* size = par + (long long)B * S;
  for (int k = 1; k < C; ++k) {
    if (!((classes >> k) & 1)) continue;
    const cc_src src{pred + (long long)k * S, (long long)C * S, 2, 0, 0.f};      // rounded values: fg = value > 0
    const int e = cc_label_sizes(src, scratch, (long long)B * S, B, H, W, D, connectivity, st);
    if (e != LTU_OK) return e;
    hipLaunchKernelGGL(cc_clear_kernel, dim3(nb, B), dim3(256), 0, st, pred, par, size, S, C, k, min_voxels);
  }
  hipLaunchKernelGGL(cc_channel0_kernel, dim3(nb, B), dim3(256), 0, st, pred, S, C);
  return ltu_check_launch();
}

// ---- largest component ---------------------------------------------------------------------------------------------------
// scratch in int32 elements: par [B][S], size [B][S], then the u64 keys best [B] (at 2 B S, an even offset)
extern "C" long long ltu_keep_largest_ws_elems(int B, int H, int W, int D) {
  if (!cc_shape_ok(B, H, W, D)) return 0;
  return (long long)B * 2 * ((long long)H * W * D + 1);
}

extern "C" int ltu_keep_largest_component(float* pred, int* scratch, long long scratch_elems, int B, int C, int H, int W, int D,
                                          int connectivity, ltu_stream_t s) {
  const int refused = cc_inplace_check(pred, scratch, scratch_elems, ltu_keep_largest_ws_elems(B, H, W, D), B, C, H, W, D, connectivity);
  if (refused != LTU_OK) return refused;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  const dim3 g((unsigned)cc_nblocks(H, W, D), B);
  int* size = scratch + (long long)B * S;
  unsigned long long* best = reinterpret_cast<unsigned long long*>(size + (long long)B * S);
  const cc_src src{pred, (long long)C * S, 4, C, 0.f, S};                       // rounded values: fg = their sum over 1 .. C-1 > 0
  const int e = cc_label_sizes(src, scratch, (long long)B * (S + 2), B, H, W, D, connectivity, st);
  if (e != LTU_OK) return e;
  hipLaunchKernelGGL(cc_pick_kernel, g, dim3(256), 0, st, size, best, S);
  hipLaunchKernelGGL(cc_keep_kernel, g, dim3(256), 0, st, pred, scratch, best, S, C);
  hipLaunchKernelGGL(cc_channel0_kernel, g, dim3(256), 0, st, pred, S, C);
  return ltu_check_launch();
}

// ---- hole filling ----------------------------------------------------------------------------------------------------------
#define CC_OPEN (-2)                              // in a root's own par slot: its component reaches a face of the volume

// every voxel of the six faces that is background of the mask marks the root of its component.  grid = (blocks, B) over
// i < 2 (W D + H D + H W); edges and corners come twice.  Every writer of a slot stores the same value, and a slot that reads
// CC_OPEN already is a marked root: no atomics.
__global__ void __launch_bounds__(256) cc_faces_kernel(int* __restrict__ par, int H, int W, int D) {
  int* pb = par + (long long)blockIdx.y * ((long long)H * W * D);
  const long long nh = (long long)W * D, nw = (long long)H * D, nd = (long long)H * W;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * (nh + nw + nd)) return;
  int h, w, d;
  if (i < 2 * nh) {
    h = i < nh ? 0 : H - 1;
    i = i < nh ? i : i - nh;
    w = (int)(i / D);
    d = (int)(i % D);
  } else if (i < 2 * (nh + nw)) {
    i -= 2 * nh;
    w = i < nw ? 0 : W - 1;
    i = i < nw ? i : i - nw;
    h = (int)(i / D);
    d = (int)(i % D);
  } else {
    i -= 2 * (nh + nw);
    d = i < nd ? 0 : D - 1;
    i = i < nd ? i : i - nd;
    h = (int)(i / W);
    w = (int)(i % W);
  }
  const int p = pb[((long long)h * W + w) * D + d];
  if (p >= 0) pb[p] = CC_OPEN;                    // p < 0: a voxel of the mask (-1), or a root that is marked already
}

// out = 1 on the mask (par -1) and on the background components without a marked root, 0 elsewhere.  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_holes_kernel(const int* __restrict__ par, uint8_t* __restrict__ out, long long S) {
  const int* pb = par + (long long)blockIdx.y * S;
  uint8_t* ob = out + (long long)blockIdx.y * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    const int p = pb[v];
    ob[v] = p == -1 ? 1 : p == CC_OPEN ? 0 : pb[p] != CC_OPEN;
  }
}

extern "C" long long ltu_fill_holes_ws_elems(int B, int H, int W, int D) {
  if (!cc_shape_ok(B, H, W, D)) return 0;
  return (long long)B * ((long long)H * W * D);
}

extern "C" int ltu_fill_holes(const uint8_t* mask, uint8_t* out, int* scratch, long long scratch_elems, int B, int H, int W, int D,
                              int connectivity, ltu_stream_t s) {
  if (!cc_shape_ok(B, H, W, D)) return LTU_E_SHAPE;
  if (connectivity < 1 || connectivity > 3 || mask == nullptr || out == nullptr) return LTU_E_ARG;
  if (scratch == nullptr || scratch_elems < ltu_fill_holes_ws_elems(B, H, W, D)) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  const long long faces = 2 * ((long long)W * D + (long long)H * D + (long long)H * W);
  const cc_src src{mask, S, 5, 0, 0.f};           // the complement: the mask is read by the labelling only, so out may be mask
  cc_label_roots(src, scratch, nullptr, B, H, W, D, connectivity, st);
  hipLaunchKernelGGL(cc_faces_kernel, dim3(cdiv(faces, 256), B), dim3(256), 0, st, scratch, H, W, D);
  hipLaunchKernelGGL(cc_holes_kernel, dim3((unsigned)cc_nblocks(H, W, D), B), dim3(256), 0, st, scratch, out, S);
  return ltu_check_launch();
}

// counts[b] += the background components of sample b whose root carries no mark: a root's slot holds its own index until
// cc_faces_kernel stores CC_OPEN there.  Integer atomics; counts zero before.  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_closed_kernel(const int* __restrict__ par, int* __restrict__ counts, long long S) {
  __shared__ int red[4];
  const int* pb = par + (long long)blockIdx.y * S;
  const long long base = (long long)blockIdx.x * CC_RB;
  int n = 0;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    n += pb[v] == (int)v;
  }
  n = cc_block_sum(n, red);
  if (threadIdx.x == 0 && n) atomicAdd(&counts[blockIdx.y], n);
}

// the cavities of a mask (its second Betti number): the 6-connected background components that reach no face of the volume, by
// the labelling and face marking of ltu_fill_holes (the same scratch, ltu_fill_holes_ws_elems), counted instead of filled
extern "C" int ltu_count_cavities(const uint8_t* mask, int* counts, int* scratch, long long scratch_elems, int B, int H, int W, int D,
                                  ltu_stream_t s) {
  if (!cc_shape_ok(B, H, W, D)) return LTU_E_SHAPE;
  if (mask == nullptr || counts == nullptr) return LTU_E_ARG;
  if (scratch == nullptr || scratch_elems < ltu_fill_holes_ws_elems(B, H, W, D)) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  const long long faces = 2 * ((long long)W * D + (long long)H * D + (long long)H * W);
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const cc_src src{mask, S, 5, 0, 0.f};
  cc_label_roots(src, scratch, nullptr, B, H, W, D, 1, st);
  hipLaunchKernelGGL(cc_faces_kernel, dim3(cdiv(faces, 256), B), dim3(256), 0, st, scratch, H, W, D);
  hipLaunchKernelGGL(cc_closed_kernel, dim3((unsigned)cc_nblocks(H, W, D), B), dim3(256), 0, st, scratch, counts, S);
  return ltu_check_launch();
}

// ---- lesion statistics ---------------------------------------------------------------------------------------------------
// v is a head of the set X (in(v) and no half-neighbour n with in(n)); in() takes a flat index inside the sample
template <int NOFF, typename In>
__device__ __forceinline__ bool cc_is_head(long long v, int H, int W, int D, In in) {
  const int d = (int)(v % D), w = (int)((v / D) % W), h = (int)(v / ((long long)W * D));
#pragma unroll
  for (int o = 0; o < NOFF; ++o) {
    const int nh = h + cc_off[o][0], nw = w + cc_off[o][1], nd = d + cc_off[o][2];
    if (nh < 0 || nw < 0 || nd < 0 || nw >= W || nd >= D) continue;
    if (in(((long long)nh * W + nw) * D + nd)) return false;
  }
  (void)H;
  return true;
}

// heads[b] += heads of P n G of sample b: a bound on the distinct (P_i, G_j) pairs, which sizes the hash set.  grid = (nb, B)
template <int NOFF>
__global__ void __launch_bounds__(256) cc_heads_kernel(cc_src P, cc_src G, int* __restrict__ heads, int H, int W, int D) {
  __shared__ int red[4];
  const int b = blockIdx.y;
  const long long S = (long long)H * W * D, base = (long long)blockIdx.x * CC_RB;
  auto both = [&](long long i) { return cc_fg(P, b, i) && cc_fg(G, b, i); };
  int n = 0;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    if (both(v) && cc_is_head<NOFF>(v, H, W, D, both)) ++n;
  }
  n = cc_block_sum(n, red);
  if (threadIdx.x == 0 && n) atomicAdd(&heads[b], n);
}

// root-indexed histograms of sample b: sp = |P_i|, sg = |G_j|, op = |P_i n G|, og = |G_j n P|.  grid = (nb, B)
__global__ void __launch_bounds__(256) cc_lesion_hist_kernel(const int* __restrict__ parp, const int* __restrict__ parg, int* __restrict__ sp,
                                                             int* __restrict__ sg, int* __restrict__ op, int* __restrict__ og, long long S) {
  const long long o = (long long)blockIdx.y * S, base = (long long)blockIdx.x * CC_RB;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    const int rp = v < S ? parp[o + v] : -1, rg = v < S ? parg[o + v] : -1;
    const bool both = rp >= 0 && rg >= 0;
    cc_wave_hist(sp + o, rp);
    cc_wave_hist(sg + o, rg);
    cc_wave_hist(op + o, both ? rp : -1);
    cc_wave_hist(og + o, both ? rg : -1);
  }
}

__device__ __forceinline__ unsigned long long cc_mix64(unsigned long long x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// distinct (root P, root G) pairs from the heads of P n G into the set tab [B][cap] (cap a power of two); each new pair adds
// |P_i| into u[G_j].  A full set (the caller's pair bound was short) counts into fail[b] instead of probing forever.
template <int NOFF>
__global__ void __launch_bounds__(256) cc_pairs_kernel(const int* __restrict__ parp, const int* __restrict__ parg, const int* __restrict__ sp,
                                                       int* __restrict__ u, unsigned long long* __restrict__ tab, long long cap,
                                                       int* __restrict__ fail, int H, int W, int D) {
  const int b = blockIdx.y;
  const long long S = (long long)H * W * D, o = (long long)b * S, base = (long long)blockIdx.x * CC_RB;
  auto both = [&](long long i) { return parp[o + i] >= 0 && parg[o + i] >= 0; };
  unsigned long long* tb = tab + (long long)b * cap;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    if (!both(v) || !cc_is_head<NOFF>(v, H, W, D, both)) continue;
    const int rp = parp[o + v], rg = parg[o + v];
    const unsigned long long key = ((unsigned long long)(unsigned)rp << 32) | (unsigned)rg;
    unsigned long long slot = cc_mix64(key) & (unsigned long long)(cap - 1);
    bool placed = false;
    for (long long probe = 0; probe < cap; ++probe) {
      const unsigned long long old = atomicCAS(&tb[slot], CC_EMPTY, key);
      if (old == CC_EMPTY) { atomicAdd(&u[o + rg], sp[o + rp]); placed = true; break; }
      if (old == key) { placed = true; break; }
      slot = (slot + 1) & (unsigned long long)(cap - 1);
    }
    if (!placed) atomicAdd(&fail[b], 1);
  }
}

__device__ __forceinline__ double cc_wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// per-block partials of sample b: pd = sum of Dice_j over the GT roots of the block (fp64, fixed order), pc[4] = n, TP, m, FP
__global__ void __launch_bounds__(256) cc_lesion_partial_kernel(const int* __restrict__ parp, const int* __restrict__ parg,
                                                                const int* __restrict__ sp, const int* __restrict__ sg,
                                                                const int* __restrict__ op, const int* __restrict__ og,
                                                                const int* __restrict__ u, double* __restrict__ pd, int* __restrict__ pc,
                                                                long long S, int nb) {
  __shared__ int red[4];
  __shared__ double dred[4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long o = (long long)b * S, base = (long long)blockIdx.x * CC_RB;
  double dice = 0.0;
  int n = 0, tp = 0, m = 0, fp = 0;
  for (int j = 0; j < CC_RB / 256; ++j) {
    const long long v = base + j * 256 + threadIdx.x;
    if (v >= S) break;
    if (parg[o + v] == (int)v) {
      const int ov = og[o + v];
      ++n;
      tp += ov > 0;
      dice += 2.0 * ov / ((double)sg[o + v] + (double)u[o + v]);
    }
    if (parp[o + v] == (int)v) {
      ++m;
      fp += op[o + v] == 0;
    }
  }
  dice = cc_wave_sum_f64(dice);
  if (lane == 0) dred[wave] = dice;
  n = cc_block_sum(n, red);
  tp = cc_block_sum(tp, red);
  m = cc_block_sum(m, red);
  fp = cc_block_sum(fp, red);
  if (threadIdx.x == 0) {
    const long long q = (long long)b * nb + blockIdx.x;
    pd[q] = ((dred[0] + dred[1]) + dred[2]) + dred[3];
    pc[4 * q] = n;
    pc[4 * q + 1] = tp;
    pc[4 * q + 2] = m;
    pc[4 * q + 3] = fp;
  }
}

// one workgroup per sample: folds the partials in a fixed order, writes column kk of ints [5][B][K] (NumTrue, NumPred,
// TruePositives, FalseNegatives, FalsePositives) and rates [4][B][K] (Sensitivity, Precision, F1, LesionDice)
__global__ void __launch_bounds__(256) cc_lesion_final_kernel(const double* __restrict__ pd, const int* __restrict__ pc,
                                                              const int* __restrict__ fail, int* __restrict__ ints,
                                                              float* __restrict__ rates, int nb, int B, int K, int kk) {
  __shared__ int red[4];
  __shared__ double dred[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double dice = 0.0;
  int c[4] = {0, 0, 0, 0};
  for (int i = threadIdx.x; i < nb; i += 256) {
    const long long q = (long long)b * nb + i;
    dice += pd[q];
    for (int t = 0; t < 4; ++t) c[t] += pc[4 * q + t];
  }
  dice = cc_wave_sum_f64(dice);
  if (lane == 0) dred[wave] = dice;
  for (int t = 0; t < 4; ++t) c[t] = cc_block_sum(c[t], red);
  if (threadIdx.x != 0) return;
  const double dsum = ((dred[0] + dred[1]) + dred[2]) + dred[3];
  const int n = c[0], tp = c[1], m = c[2], fp = c[3];
  const long long at = (long long)b * K + kk, plane = (long long)B * K;
  if (fail[b] != 0) {                              // the pair bound the caller gave was short: no value rather than a wrong one
    for (int t = 0; t < 5; ++t) ints[t * plane + at] = -1;
    for (int t = 0; t < 4; ++t) rates[t * plane + at] = __builtin_nanf("");
    return;
  }
  const double sens = n == 0 ? 1.0 : (double)tp / n;
  const double prec = m == 0 ? 1.0 : (double)(m - fp) / m;
  const double f1 = sens + prec == 0.0 ? 0.0 : 2.0 * sens * prec / (sens + prec);
  const double ld = n + fp == 0 ? 1.0 : dsum / (n + fp);
  ints[at] = n;
  ints[plane + at] = m;
  ints[2 * plane + at] = tp;
  ints[3 * plane + at] = n - tp;
  ints[4 * plane + at] = fp;
  rates[at] = (float)sens;
  rates[plane + at] = (float)prec;
  rates[2 * plane + at] = (float)f1;
  rates[3 * plane + at] = (float)ld;
}

// hash-set capacity for a pair bound: a power of two >= 2 * pairs, at least 64
static long long cc_hash_cap(long long pairs) {
  long long cap = 64;
  while (cap < 2 * pairs) cap <<= 1;
  return cap;
}

// scratch layout of ltu_lesion_stats in 4-byte elements: par P, par G, then sp sg op og u (root-indexed, zeroed per call),
// partial Dice (doubles), partial counts, fail, the hash set (u64); 8-byte arrays at even offsets
struct cc_lesion_layout {
  long long parp, parg, stats, pd, pc, fail, tab, total, cap;
};

static cc_lesion_layout cc_lesion_plan(int B, int H, int W, int D, long long pairs) {
  const long long BS = (long long)B * H * W * D, nb = cc_nblocks(H, W, D);
  cc_lesion_layout l;
  l.cap = cc_hash_cap(pairs);
  l.parp = 0;
  l.parg = BS;
  l.stats = 2 * BS;
  l.pd = (7 * BS + 1) / 2 * 2;
  l.pc = l.pd + 2 * B * nb;
  l.fail = l.pc + 4 * B * nb;
  l.tab = (l.fail + B + 1) / 2 * 2;
  l.total = l.tab + 2 * B * l.cap;
  return l;
}

extern "C" long long ltu_lesion_ws_elems(int B, int H, int W, int D, long long pairs) {
  if (!cc_shape_ok(B, H, W, D) || pairs < 0 || pairs > (long long)H * W * D) return 0;
  return cc_lesion_plan(B, H, W, D, pairs).total;
}

static bool cc_lesion_args_ok(const float* pred, const uint8_t* target, int C, int k, float threshold, int connectivity) {
  return pred != nullptr && target != nullptr && k >= 0 && k < C && k < 256 && threshold == threshold && connectivity >= 1 &&
         connectivity <= 3;
}

extern "C" int ltu_lesion_heads(const float* pred, const uint8_t* target, int* heads, int B, int C, int k, int H, int W, int D,
                                float threshold, int connectivity, ltu_stream_t s) {
  if (!cc_shape_ok(B, H, W, D) || C < 1) return LTU_E_SHAPE;
  if (!cc_lesion_args_ok(pred, target, C, k, threshold, connectivity) || heads == nullptr) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D;
  const int nb = (int)cc_nblocks(H, W, D);
  const cc_src P{pred + (long long)k * S, (long long)C * S, 1, 0, threshold}, G{target, S, 3, k, 0.f};
  const hipError_t e = hipMemsetAsync(heads, 0, (size_t)B * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const dim3 g(nb, B);
  if (connectivity == 1) hipLaunchKernelGGL(cc_heads_kernel<3>, g, dim3(256), 0, st, P, G, heads, H, W, D);
  else if (connectivity == 2) hipLaunchKernelGGL(cc_heads_kernel<9>, g, dim3(256), 0, st, P, G, heads, H, W, D);
  else hipLaunchKernelGGL(cc_heads_kernel<13>, g, dim3(256), 0, st, P, G, heads, H, W, D);
  return ltu_check_launch();
}

extern "C" int ltu_lesion_stats(const float* pred, const uint8_t* target, int* ints, float* rates, void* scratch,
                                long long scratch_elems, long long pairs, int B, int C, int k, int kk, int K, int H, int W, int D,
                                float threshold, int connectivity, ltu_stream_t s) {
  if (!cc_shape_ok(B, H, W, D) || C < 1 || K < 1 || kk < 0 || kk >= K) return LTU_E_SHAPE;
  if (!cc_lesion_args_ok(pred, target, C, k, threshold, connectivity) || ints == nullptr || rates == nullptr) return LTU_E_ARG;
  if (pairs < 0 || scratch == nullptr || scratch_elems < ltu_lesion_ws_elems(B, H, W, D, pairs)) return LTU_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const long long S = (long long)H * W * D, BS = (long long)B * S;
  const int nb = (int)cc_nblocks(H, W, D);
  const cc_lesion_layout l = cc_lesion_plan(B, H, W, D, pairs);
  int* base = static_cast<int*>(scratch);
  int *parp = base + l.parp, *parg = base + l.parg, *sp = base + l.stats, *sg = sp + BS, *op = sg + BS, *og = op + BS, *u = og + BS;
  double* pd = reinterpret_cast<double*>(base + l.pd);
  int* pc = base + l.pc;
  int* fail = base + l.fail;
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(base + l.tab);
  const cc_src P{pred + (long long)k * S, (long long)C * S, 1, 0, threshold}, G{target, S, 3, k, 0.f};
  cc_label_roots(P, parp, nullptr, B, H, W, D, connectivity, st);
  cc_label_roots(G, parg, nullptr, B, H, W, D, connectivity, st);
  hipError_t e = hipMemsetAsync(sp, 0, (size_t)5 * BS * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(fail, 0, (size_t)B * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(tab, 0xff, (size_t)B * l.cap * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  const dim3 g(nb, B);
  hipLaunchKernelGGL(cc_lesion_hist_kernel, g, dim3(256), 0, st, parp, parg, sp, sg, op, og, S);
  if (connectivity == 1) hipLaunchKernelGGL(cc_pairs_kernel<3>, g, dim3(256), 0, st, parp, parg, sp, u, tab, l.cap, fail, H, W, D);
  else if (connectivity == 2) hipLaunchKernelGGL(cc_pairs_kernel<9>, g, dim3(256), 0, st, parp, parg, sp, u, tab, l.cap, fail, H, W, D);
  else hipLaunchKernelGGL(cc_pairs_kernel<13>, g, dim3(256), 0, st, parp, parg, sp, u, tab, l.cap, fail, H, W, D);
  hipLaunchKernelGGL(cc_lesion_partial_kernel, g, dim3(256), 0, st, parp, parg, sp, sg, op, og, u, pd, pc, S, nb);
  hipLaunchKernelGGL(cc_lesion_final_kernel, dim3(B), dim3(256), 0, st, pd, pc, fail, ints, rates, nb, B, K, kk);
  return ltu_check_launch();
}
