// Surface-distance metrics of a segmentation (evaluation side, no reference counterpart): Hausdorff distance, its 95th
// percentile, the average symmetric surface distance and normalised surface Dice, per (sample, class).
//
// Definition (the same words are in include/ltu_hip.h and infer.surface_metrics):
//   A = pred[b][k] >= threshold, B = target[b] == k (integer labels).  The boundary dX holds the voxels of X with at least one
//   of their 6 face neighbours outside X; voxels beyond the volume count as outside (X & ~binary_erosion(X, 6-cross,
//   border_value=0)).  d(x, dY) = min over y in dY of sqrt(sum_i ((x_i - y_i) s_i)^2), s = (s_H, s_W, s_D) the spacing.
//   DA = {d(a, dB) : a in dA}, DB = {d(b, dA) : b in dB};
//   HD = max(max DA, max DB), HD95 = max(P95(DA), P95(DB)) (numpy's default linear percentile), ASSD = (sum DA + sum DB) /
//   (|dA| + |dB|), NSD(tau) = (#{DA <= tau} + #{DB <= tau}) / (|dA| + |dB|) - the boundary-voxel-count form of NSD, not the
//   surfel-area form.  Both boundaries empty: 0 / 0 / 0 / 1; exactly one empty: inf / inf / inf / 0.
//
// Phases (one entry point each):
//   1. ltu_surface_boundary: dA (bit 0) and dB (bit 1) of every voxel in one pass, plus the bounding box of dA u dB through a
//      per-workgroup LDS reduction and one integer atomic min / max per workgroup (order-independent).
//   2. ltu_surface_edt: exact squared EDT of both boundaries over the crop = that box (exact: every source lies inside it, and
//      only boundary voxels, also inside it, are queried).  Separable: along H the 1-D nearest-source distance (two sweeps),
//      along W and D the lower envelope of parabolas min_i (s^2 (q - i)^2 + g(i)) by Felzenszwalb-Huttenlocher, one lane per
//      line, any line length (the envelope lives in global scratch laid out [i][line], so neighbouring lanes touch neighbouring
//      words).  Intersections are computed in fp64; with unit spacing every value is an integer below 2^24 and exact in fp32.
//   3. ltu_surface_stats: count, max, #<=tau and the fp64 sum of each direction from per-workgroup partials folded in a fixed
//      order (no float atomics: two calls give bit-identical results), then the floor / ceil order statistics of the 95th
//      percentile of each direction by an 8-bit radix select over the fp32 bit patterns (non-negative floats order like their
//      bits): four histogram passes with integer atomics, each followed by a one-workgroup pick.
//   4. ltu_surface_finalize: the four metrics of every (sample, class) from the per-pair records, empty-set rules included.
#include "common.h"

#include <math.h>

#define SURF_INF __builtin_inff()

static unsigned surf_grid(long long n, int per_block = 256) {
  long long blocks = (n + per_block - 1) / per_block;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// ------------------------------------------------------------------------------------------------ 1. boundaries + box
__global__ void surf_box_init_kernel(int* __restrict__ bbox, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * B) bbox[i] = (i % 6) < 3 ? 0x7FFFFFFF : -1;
}

// edges [B][H][W][D]: bit 0 = voxel of dA, bit 1 = voxel of dB.  bbox [B][6] = (min h, w, d, max h, w, d) of dA u dB, max < 0
// when both are empty.  grid.y = sample.
__global__ void __launch_bounds__(256) surf_boundary_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ target,
                                                            uint8_t* __restrict__ edges, int* __restrict__ bbox, int C, int k, int H,
                                                            int W, int D, float thr) {
  __shared__ int box[6];
  if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? 0x7FFFFFFF : -1;
  __syncthreads();
  const int b = blockIdx.y;
  const long long S = (long long)H * W * D, WD = (long long)W * D;
  const float* p = pred + ((long long)b * C + k) * S;
  const uint8_t* t = target + (long long)b * S;
  int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
    const int z = (int)(i % D), y = (int)((i / D) % W), x = (int)(i / WD);
    const bool a = p[i] >= thr, m = t[i] == (uint8_t)k;
    bool ea = false, em = false;
    if (a || m) {
      // a face neighbour outside the set (or outside the volume) makes the voxel a boundary voxel
      const long long nb[6] = {i - WD, i + WD, i - D, i + D, i - 1, i + 1};
      const bool in[6] = {x > 0, x + 1 < H, y > 0, y + 1 < W, z > 0, z + 1 < D};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        ea |= a && (!in[j] || !(p[in[j] ? nb[j] : i] >= thr));
        em |= m && (!in[j] || t[in[j] ? nb[j] : i] != (uint8_t)k);
      }
    }
    const uint8_t e = (uint8_t)((ea ? 1 : 0) | (em ? 2 : 0));
    edges[(long long)b * S + i] = e;
    if (e) {
      lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
      hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
    }
  }
  if (hi[0] >= 0) {
    for (int j = 0; j < 3; ++j) { atomicMin(box + j, lo[j]); atomicMax(box + 3 + j, hi[j]); }
  }
  __syncthreads();
  if (threadIdx.x < 6 && box[3] >= 0) {
    if (threadIdx.x < 3) atomicMin(bbox + 6 * b + threadIdx.x, box[threadIdx.x]);
    else atomicMax(bbox + 6 * b + threadIdx.x, box[threadIdx.x]);
  }
}

// ------------------------------------------------------------------------------------------------ 2. squared EDT over the crop
// dist [2][h][w][d]: channel c = squared distance to the voxels of bit c, along H only: (s_H * |h - nearest|)^2, +inf without one.
// One lane per (c, w, d) column; lanes run along d, so every step reads and writes contiguous words.
__global__ void __launch_bounds__(256) surf_edt_h_kernel(const uint8_t* __restrict__ edges, float* __restrict__ dist, int W, int D,
                                                         int h0, int w0, int d0, int h, int w, int d, float sh) {
  const long long cols = (long long)w * d, total = 2 * cols;
  const double s2 = (double)sh * sh;
  for (long long L = (long long)blockIdx.x * blockDim.x + threadIdx.x; L < total; L += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(L / cols);
    const long long r = L - c * cols;
    const int yy = (int)(r / d), zz = (int)(r % d);
    const uint8_t bit = (uint8_t)(1 << c);
    const uint8_t* e = edges + ((long long)h0 * W + (w0 + yy)) * D + (d0 + zz);
    float* o = dist + (long long)c * h * cols + r;
    int last = -1;
    for (int x = 0; x < h; ++x) {            // forward: distance (in voxels) to the nearest source at or before x
      if (e[(long long)x * W * D] & bit) last = x;
      o[x * cols] = last >= 0 ? (float)(x - last) : SURF_INF;
    }
    int next = -1;
    for (int x = h - 1; x >= 0; --x) {       // backward: the nearer of the two, squared and scaled
      if (e[(long long)x * W * D] & bit) next = x;
      float v = o[x * cols];
      if (next >= 0 && (float)(next - x) < v) v = (float)(next - x);
      o[x * cols] = v < SURF_INF ? (float)(s2 * (double)v * (double)v) : SURF_INF;
    }
  }
}

// one line of n elements at line[i * stride]: g(q) <- min_i (s2 (q - i)^2 + g(i)), in place (Felzenszwalb-Huttenlocher).  The
// envelope's parabola apexes v[] and their values fv[] sit in scratch at [j * nlines + L].
__global__ void __launch_bounds__(256) surf_edt_fh_kernel(float* __restrict__ dist, int* __restrict__ vs, float* __restrict__ fvs,
                                                          long long nlines, int n, long long inner, float sp) {
  const double s2 = (double)sp * sp;
  for (long long L = (long long)blockIdx.x * blockDim.x + threadIdx.x; L < nlines; L += (long long)gridDim.x * blockDim.x) {
    float* line = dist + (L / inner) * ((long long)n * inner) + (L % inner);
    int* v = vs + L;
    float* fv = fvs + L;
    // intersection abscissa of the parabolas with apexes (p, gp) and (q, gq), p < q
    auto cross = [&](int p, double gp, int q, double gq) {
      return ((gq + s2 * (double)q * q) - (gp + s2 * (double)p * p)) / (2.0 * s2 * (double)(q - p));
    };
    int k = -1;
    double ztop = -(double)SURF_INF;          // left end of the top parabola's interval
    for (int i = 0; i < n; ++i) {
      const float f = line[(long long)i * inner];
      if (!(f < SURF_INF)) continue;
      double zi = -(double)SURF_INF;
      while (k >= 0) {
        zi = cross(v[(long long)k * nlines], fv[(long long)k * nlines], i, f);
        if (zi > ztop) break;
        --k;                                  // the top parabola is nowhere lowest: pop it
        ztop = k > 0 ? cross(v[(long long)(k - 1) * nlines], fv[(long long)(k - 1) * nlines], v[(long long)k * nlines],
                             fv[(long long)k * nlines])
                     : -(double)SURF_INF;
        zi = -(double)SURF_INF;
      }
      ++k;
      v[(long long)k * nlines] = i;
      fv[(long long)k * nlines] = f;
      ztop = zi;
    }
    if (k < 0) {                              // no source on this line
      for (int q = 0; q < n; ++q) line[(long long)q * inner] = SURF_INF;
      continue;
    }
    int j = 0, vj = v[0];
    double fj = fv[0];
    double znext = k > 0 ? cross(vj, fj, v[nlines], fv[nlines]) : (double)SURF_INF;
    for (int q = 0; q < n; ++q) {
      while (j < k && znext < (double)q) {
        ++j;
        vj = v[(long long)j * nlines];
        fj = fv[(long long)j * nlines];
        znext = j < k ? cross(vj, fj, v[(long long)(j + 1) * nlines], fv[(long long)(j + 1) * nlines]) : (double)SURF_INF;
      }
      const double dq = (double)(q - vj);
      line[(long long)q * inner] = (float)(s2 * dq * dq + fj);
    }
  }
}

// ------------------------------------------------------------------------------------------------ 3. directed statistics
#define SURF_STATS_BLOCKS 256
#define SURF_REC 12             // per-pair record (doubles): see ltu_surface_stats in include/ltu_hip.h

// one crop voxel: dA (distance of a voxel of dA to dB) and / or dB, as fp32
struct SurfVoxel {
  bool a, b;
  float da, db;
};
__device__ __forceinline__ SurfVoxel surf_voxel(const uint8_t* __restrict__ edges, const float* __restrict__ dist, long long r,
                                                long long V, int W, int D, int h0, int w0, int d0, int w, int d) {
  const int zz = (int)(r % d), yy = (int)((r / d) % w), xx = (int)(r / ((long long)w * d));
  const uint8_t e = edges[((long long)(h0 + xx) * W + (w0 + yy)) * D + (d0 + zz)];
  SurfVoxel s;
  s.a = e & 1;
  s.b = (e >> 1) & 1;
  s.da = s.a ? sqrtf(dist[V + r]) : 0.f;     // channel 1 = squared distance to dB
  s.db = s.b ? sqrtf(dist[r]) : 0.f;         // channel 0 = squared distance to dA
  return s;
}

// part [G][8] doubles: count A, count B, max A, max B, sum A, sum B, #<=tau A, #<=tau B of the workgroup's voxels
__global__ void __launch_bounds__(256) surf_stats_partial_kernel(const uint8_t* __restrict__ edges, const float* __restrict__ dist,
                                                                 double* __restrict__ part, long long V, int W, int D, int h0, int w0,
                                                                 int d0, int w, int d, float tau) {
  __shared__ double red[8][256];
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < V; r += (long long)gridDim.x * blockDim.x) {
    const SurfVoxel s = surf_voxel(edges, dist, r, V, W, D, h0, w0, d0, w, d);
    if (s.a) { a[0] += 1; a[2] = fmax(a[2], (double)s.da); a[4] += s.da; a[6] += s.da <= tau ? 1 : 0; }
    if (s.b) { a[1] += 1; a[3] = fmax(a[3], (double)s.db); a[5] += s.db; a[7] += s.db <= tau ? 1 : 0; }
  }
  for (int j = 0; j < 8; ++j) red[j][threadIdx.x] = a[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int j = 0; j < 8; ++j)
        red[j][threadIdx.x] = (j == 2 || j == 3) ? fmax(red[j][threadIdx.x], red[j][threadIdx.x + o])
                                                 : red[j][threadIdx.x] + red[j][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 8) part[blockIdx.x * 8 + threadIdx.x] = red[threadIdx.x][0];
}

// select state [4][2] ints = (prefix bits found so far, rank still to skip) of: A floor, A ceil, B floor, B ceil
__device__ __forceinline__ void surf_p95_ranks(double n, long long* lo, long long* hi) {
  const double pos = (n - 1.0) * 0.95;                       // numpy: (n - 1) * quantile, quantile = 95 / 100
  *lo = (long long)floor(pos);
  *hi = *lo + 1 < (long long)n ? *lo + 1 : (long long)n - 1;
}

// fold of the partials in workgroup order (one lane per field); the rank of each order statistic; hist zeroed
__global__ void __launch_bounds__(256) surf_stats_fold_kernel(const double* __restrict__ part, int G, double* __restrict__ rec,
                                                              int* __restrict__ state, int* __restrict__ hist) {
  for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) hist[i] = 0;
  __shared__ double tot[8];
  if (threadIdx.x < 8) {
    const int j = threadIdx.x;
    double acc = 0.0;
    for (int g = 0; g < G; ++g) acc = (j == 2 || j == 3) ? fmax(acc, part[g * 8 + j]) : acc + part[g * 8 + j];
    tot[j] = acc;
    rec[j] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double n = tot[threadIdx.x];
    long long lo = 0, hi = 0;
    if (n > 0) surf_p95_ranks(n, &lo, &hi);
    state[(2 * threadIdx.x) * 2] = 0; state[(2 * threadIdx.x) * 2 + 1] = (int)lo;
    state[(2 * threadIdx.x + 1) * 2] = 0; state[(2 * threadIdx.x + 1) * 2 + 1] = (int)hi;
  }
}

// hist [4][256]: per selection, the count of candidate keys (bits above `shift` equal to the prefix) by their byte at `shift`
__global__ void __launch_bounds__(256) surf_radix_hist_kernel(const uint8_t* __restrict__ edges, const float* __restrict__ dist,
                                                              const int* __restrict__ state, int* __restrict__ hist, long long V,
                                                              int W, int D, int h0, int w0, int d0, int w, int d, int shift) {
  __shared__ int h[4][256];
  for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) (&h[0][0])[i] = 0;
  __syncthreads();
  const unsigned mask = shift >= 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
  unsigned pre[4];
  for (int j = 0; j < 4; ++j) pre[j] = (unsigned)state[2 * j];
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < V; r += (long long)gridDim.x * blockDim.x) {
    const SurfVoxel s = surf_voxel(edges, dist, r, V, W, D, h0, w0, d0, w, d);
    if (s.a) {
      const unsigned key = __float_as_uint(s.da), bin = (key >> shift) & 255u;
      if ((key & mask) == pre[0]) atomicAdd(&h[0][bin], 1);
      if ((key & mask) == pre[1]) atomicAdd(&h[1][bin], 1);
    }
    if (s.b) {
      const unsigned key = __float_as_uint(s.db), bin = (key >> shift) & 255u;
      if ((key & mask) == pre[2]) atomicAdd(&h[2][bin], 1);
      if ((key & mask) == pre[3]) atomicAdd(&h[3][bin], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) {
    const int c = (&h[0][0])[i];
    if (c) atomicAdd(hist + i, c);
  }
}

// one lane per selection: the bin that holds the wanted rank joins the prefix; hist is zeroed for the next pass.  After the
// last pass (shift 0) the prefix is the key: rec[8 + j] = that value.
__global__ void __launch_bounds__(64) surf_radix_pick_kernel(int* __restrict__ state, int* __restrict__ hist, double* __restrict__ rec,
                                                             int shift) {
  const int j = threadIdx.x;
  if (j < 4) {
    int rank = state[2 * j + 1], cum = 0, bin = 0;
    for (; bin < 256; ++bin) {
      const int c = hist[j * 256 + bin];
      if (rank < cum + c) break;
      cum += c;
    }
    if (bin < 256) {                          // no candidates (empty direction): the state is not used
      state[2 * j] = (int)((unsigned)state[2 * j] | ((unsigned)bin << shift));
      state[2 * j + 1] = rank - cum;
    }
    if (shift == 0) rec[8 + j] = (double)__uint_as_float((unsigned)state[2 * j]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) hist[i] = 0;
}

// ------------------------------------------------------------------------------------------------ 4. the metrics
__device__ __forceinline__ double surf_lerp(double a, double b, double t) {   // numpy's _lerp
  const double diff = b - a;
  return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}
__device__ __forceinline__ double surf_p95(double n, double lo_v, double hi_v) {
  const double pos = (n - 1.0) * 0.95;
  return surf_lerp(lo_v, hi_v, pos - floor(pos));
}

// out [4][B][K] = HD, HD95, ASSD, NSD; pair q = kk * B + b
__global__ void surf_finalize_kernel(const double* __restrict__ rec, float* __restrict__ out, int B, int K) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int P = B * K;
  if (q >= P) return;
  const double* r = rec + (long long)q * SURF_REC;
  const int kk = q / B, b = q % B;
  const double na = r[0], nb = r[1];
  float hd, hd95, assd, nsd;
  if (na == 0 && nb == 0) {
    hd = hd95 = assd = 0.f; nsd = 1.f;
  } else if (na == 0 || nb == 0) {
    hd = hd95 = assd = SURF_INF; nsd = 0.f;
  } else {
    hd = (float)fmax(r[2], r[3]);
    hd95 = (float)fmax(surf_p95(na, r[8], r[9]), surf_p95(nb, r[10], r[11]));
    assd = (float)((r[4] + r[5]) / (na + nb));
    nsd = (float)((r[6] + r[7]) / (na + nb));
  }
  const long long o = (long long)b * K + kk, st = (long long)B * K;
  out[o] = hd;
  out[st + o] = hd95;
  out[2 * st + o] = assd;
  out[3 * st + o] = nsd;
}

// ------------------------------------------------------------------------------------------------ host
static bool surf_box_ok(int H, int W, int D, int h0, int w0, int d0, int h, int w, int d) {
  return H > 0 && W > 0 && D > 0 && h > 0 && w > 0 && d > 0 && h0 >= 0 && w0 >= 0 && d0 >= 0 && h0 + h <= H && w0 + w <= W &&
         d0 + d <= D;
}
static long long surf_stats_elems(int G) { return 16LL * G + 4 * 256 + 8; }

extern "C" int ltu_surface_boundary(const float* pred, const uint8_t* target, uint8_t* edges, int* bbox, int B, int C, int k, int H,
                                    int W, int D, float threshold, ltu_stream_t s) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0 || B > 65535) return LTU_E_SHAPE;
  if (k < 0 || k >= C || k > 255) return LTU_E_ARG;
  const long long S = (long long)H * W * D;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(surf_box_init_kernel, dim3(cdiv(6LL * B, 256)), dim3(256), 0, st, bbox, B);
  hipLaunchKernelGGL(surf_boundary_kernel, dim3(surf_grid(S), B), dim3(256), 0, st, pred, target, edges, bbox, C, k, H, W, D, threshold);
  return ltu_check_launch();
}

extern "C" long long ltu_surface_ws_elems(int h, int w, int d) {
  const long long edt = 4LL * h * w * d, stats = surf_stats_elems(SURF_STATS_BLOCKS);
  return edt > stats ? edt : stats;
}

extern "C" int ltu_surface_edt(const uint8_t* edges, float* dist, void* scratch, long long scratch_elems, int H, int W, int D, int h0,
                               int w0, int d0, int h, int w, int d, float sh, float sw, float sd, ltu_stream_t s) {
  if (!surf_box_ok(H, W, D, h0, w0, d0, h, w, d)) return LTU_E_SHAPE;
  if (!(sh > 0.f) || !(sw > 0.f) || !(sd > 0.f) || !(sh < SURF_INF) || !(sw < SURF_INF) || !(sd < SURF_INF)) return LTU_E_ARG;
  const long long V = (long long)h * w * d;
  if (scratch == nullptr || scratch_elems < 4 * V) return LTU_E_ARG;
  int* vs = (int*)scratch;
  float* fvs = (float*)scratch + 2 * V;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(surf_edt_h_kernel, dim3(surf_grid(2LL * w * d)), dim3(256), 0, st, edges, dist, W, D, h0, w0, d0, h, w, d, sh);
  const long long lines_w = 2LL * h * d, lines_d = 2LL * h * w;
  hipLaunchKernelGGL(surf_edt_fh_kernel, dim3(surf_grid(lines_w)), dim3(256), 0, st, dist, vs, fvs, lines_w, w, (long long)d, sw);
  hipLaunchKernelGGL(surf_edt_fh_kernel, dim3(surf_grid(lines_d)), dim3(256), 0, st, dist, vs, fvs, lines_d, d, 1LL, sd);
  return ltu_check_launch();
}

extern "C" int ltu_surface_stats(const uint8_t* edges, const float* dist, double* rec, void* scratch, long long scratch_elems, int H,
                                 int W, int D, int h0, int w0, int d0, int h, int w, int d, float tau, ltu_stream_t s) {
  if (!surf_box_ok(H, W, D, h0, w0, d0, h, w, d)) return LTU_E_SHAPE;
  if (tau != tau) return LTU_E_ARG;
  const long long V = (long long)h * w * d;
  const int G = (int)(V / 256 + 1 < SURF_STATS_BLOCKS ? V / 256 + 1 : SURF_STATS_BLOCKS);
  if (scratch == nullptr || scratch_elems < surf_stats_elems(G)) return LTU_E_ARG;
  double* part = (double*)scratch;                         // [G][8]
  int* hist = (int*)(part + 8LL * G);                      // [4][256]
  int* state = hist + 4 * 256;                             // [4][2]
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(surf_stats_partial_kernel, dim3(G), dim3(256), 0, st, edges, dist, part, V, W, D, h0, w0, d0, w, d, tau);
  hipLaunchKernelGGL(surf_stats_fold_kernel, dim3(1), dim3(256), 0, st, part, G, rec, state, hist);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(surf_radix_hist_kernel, dim3(G), dim3(256), 0, st, edges, dist, state, hist, V, W, D, h0, w0, d0, w, d, shift);
    hipLaunchKernelGGL(surf_radix_pick_kernel, dim3(1), dim3(64), 0, st, state, hist, rec, shift);
  }
  return ltu_check_launch();
}

extern "C" int ltu_surface_finalize(const double* rec, float* out, int B, int K, ltu_stream_t s) {
  if (B <= 0 || K <= 0) return LTU_E_SHAPE;
  hipLaunchKernelGGL(surf_finalize_kernel, dim3(cdiv((long long)B * K, 256)), dim3(256), 0, (hipStream_t)s, rec, out, B, K);
  return ltu_check_launch();
}
